// fa_engine.hip -- host side of libfastani_hip.so: owns the HIP stream and all HBM allocations, drives the
// kernels of fa_sketch.hip.h / fa_map.hip.h, and exports the C ABI declared in include/fastani_hip.h.  The reductions over
// finished results (pairs, clusters, representatives, best hits, the signature screen) are driven from fa_reduce.hip.h;
// this file only wraps them in their entry points.
// There is no CPU fallback anywhere in this file: without a HIP device every compute entry point fails.
#include <cstring>   // (before rocPRIM, whose texture_cache_iterator.hpp calls memset without including it)

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <memory>
#include <condition_variable>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <utility>
#include <vector>
#include <cstddef>
#include <deque>

#include "fa_common.h"
#include "fa_fasta.h"
#include "fa_ingest.h"
#include "fa_knobs.h"
#include "fa_lease.h"
#include "fa_map.hip.h"
#include "fa_policy.h"
#include "fa_sketch.hip.h"
#include "fa_sketch_fast.hip.h"
#include "fa_stats.h"
#include "fa_table.hip.h"
#include "fa_order.h"
#include "fa_represent.hip.h"
#include "fa_best.hip.h"
#include "fa_screen.hip.h"
#include "fa_reduce.hip.h"
#include "fa_select.hip.h"

using namespace fa;

// ------------------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

template <typename F>
static int guarded(F &&fn) {
  try {
    fn();
    return FA_OK;
  } catch (const Error &e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::bad_alloc &) {
    g_last_error = "host allocation failed";
    return FA_ERR_NOMEM;
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return FA_ERR_INTERNAL;
  }
}

// The device chosen with fa_set_device (-1: whatever the calling thread has current).  HIP's current device is a
// per-thread setting, and sketches / mappers are used from any host thread: each object remembers its device and every
// entry point binds it again.
static std::atomic<int> g_device{-1};
static void bind_device(int device) {
  if (device >= 0) FA_HIP(hipSetDevice(device));
}

static void validate_params(const fa_params &p) {
  FA_REQUIRE(p.kmer_size >= 1 && p.kmer_size <= 2048, FA_ERR_INVALID, "kmer_size must be in [1, 2048]");
  FA_REQUIRE(p.fragment_length >= 1, FA_ERR_INVALID, "fragment_length must be strictly positive");
  FA_REQUIRE(p.window_size >= 1, FA_ERR_INVALID, "window_size must be strictly positive");
  FA_REQUIRE(p.alphabet_size == 4 || p.alphabet_size == 20, FA_ERR_INVALID, "alphabet_size must be 4 or 20");
  size_t lds = sketch_lds_bytes(p.kmer_size, p.window_size);
  FA_REQUIRE(lds <= 160 * 1024, FA_ERR_UNSUPPORTED,
             "window_size/kmer_size too large for the LDS-staged sketch kernel (tile + 2w + k must fit 160 KiB)");
}

// launches `kernel` with `lds` bytes of dynamic LDS; above 64 KB the kernel has to be allowed them first
template <typename Kernel, typename... Args>
static void launch_lds(Kernel kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &...args) {
  if (lds > 64 * 1024) FA_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
}

// ------------------------------------------------------------------------------------------------------------
// K1 launcher shared by the reference and the query side
// ------------------------------------------------------------------------------------------------------------
struct SketchWork {
  DevBuf<Tile> tiles;
  DevBuf<uint32_t> stage_hash;
  DevBuf<int32_t> stage_wpos;
  DevBuf<int32_t> tile_count;   // ntiles + 1
  DevBuf<int32_t> tile_off;     // ntiles + 1
  DevBuf<unsigned char> cub_temp;
};

// FA_TRACE=1: wall-clock of the host-visible stages of sketching and index construction on stderr
struct StageTrace {
  bool on, live = false;
  const char *what;
  std::chrono::steady_clock::time_point t0, t;
  std::vector<std::pair<std::string, double>> acc;
  explicit StageTrace(const char *w) : what(w) {
    const double level = knob::trace();
    on = !knob::unset(level);
    live = on && level >= 2;
    t0 = t = std::chrono::steady_clock::now();
  }
  void mark(const char *stage, hipStream_t st) {
    if (!on) return;
    (void)hipStreamSynchronize(st);
    auto now = std::chrono::steady_clock::now();
    double ms = std::chrono::duration<double, std::milli>(now - t).count();
    t = now;
    if (live) { fprintf(stderr, "[fa trace] %s: %s done after %.1f ms\n", what, stage, ms); fflush(stderr); }   // FA_TRACE=2: as it happens
    for (auto &a : acc) if (a.first == stage) { a.second += ms; return; }
    acc.emplace_back(stage, ms);
  }
  ~StageTrace() {
    if (!on) return;
    fprintf(stderr, "[fa trace] %s: %.1f ms total;", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    for (auto &a : acc) fprintf(stderr, " %s %.1f", a.first.c_str(), a.second);
    fprintf(stderr, "\n");
  }
};

// `clear` (a query pass): ranges zeroed by extra workgroups of the first launch, beside the hashing
// `fuse` (a query pass, F fragments): K1 and the per-fragment sketch in one launch (k_query_fused) where the pass qualifies
// -- returns true then, and the caller skips k_query_sketch
static bool launch_sketch_tiles(const fa_params &P, const StoreView &store, const Tile *d_tiles, int ntiles, uint32_t *stage_hash,
                                int32_t *stage_wpos, int32_t *tile_count, hipStream_t st, const ClearArgs *clear = nullptr,
                                const QuerySketchArgs *fuse = nullptr, int64_t F = 0) {
  if (ntiles <= 0) {
    if (clear && clear->count) hipLaunchKernelGGL(k_clear, dim3(256), dim3(256), 0, st, *clear);
    return false;
  }
  SketchArgs a;
  a.ntiles = ntiles;
  a.clear.count = 0; a.clear.stamp = nullptr;
  int extra = 0;
  if (clear && clear->count) {
    a.clear = *clear;
    uint64_t most = 0;
    for (int i = 0; i < clear->count; i++) most = std::max(most, clear->n16[i]);
    extra = (int)std::min<uint64_t>(512, std::max<uint64_t>(1, (most + SK_THREADS * 8 - 1) / (SK_THREADS * 8)));
  }
  a.tiles = d_tiles;
  a.packed = store.packed; a.bytes = store.bytes; a.exc_pos = store.exc_pos; a.exc_val = store.exc_val;
  a.stage_hash = stage_hash; a.stage_wpos = stage_wpos; a.tile_count = tile_count;
  a.k = P.kmer_size; a.w = P.window_size; a.levels = floor_log2(P.window_size);
  a.protein = P.alphabet_size != 4;
  a.npos_cap = TILE + 2 * P.window_size - 2;
  // FA_K1_GENERAL=1: every tile through the 64-bit form of the window minimum (tests compare the two)
  const bool k1_general = knob::k1_general() != 0;
  a.fast = (!k1_general && P.window_size >= 3 && P.window_size <= 1000) ? 1 : 0;   // (three padded arrays in the LDS of two key arrays)
  size_t lds = sketch_lds_bytes(P.kmer_size, P.window_size);
  size_t image = lds - ((size_t)a.npos_cap * 16 + ((size_t)a.npos_cap / 64 + 1) * 8 + (TILE / 64) * 8 + (TILE / 64 + 1) * 4 + 16 + 4 * 256 * 8);
  a.code_words = (int32_t)(image / 4);
  auto launch = [&](auto kernel) {
    launch_lds(kernel, dim3(ntiles + extra), dim3(SK_THREADS), lds, st, a);
    extra = 0; a.clear.count = 0; a.clear.stamp = nullptr;          // (only the first launch zeroes)
  };
  // plain-ACGT tiles from the 2-bit image; protein tiles and tiles with other bytes through the byte image
  if (!a.protein && !k1_general && P.window_size >= SKF_MIN_W && P.window_size <= SKF_MAX_W) {
    // the hot form (fa_sketch_fast.hip.h): 13 KB of LDS, eight workgroups per CU; k = 14 / 16 / 21 hash from the premix tables
    const size_t flds = skf_layout(P.kmer_size, P.window_size).total;
    // The (k, w) cells of the default identity cut-off over the usual fragment lengths -- BASELINE config 5's grid: k in
    // {14, 16, 21} x fragment in {1000, 3000, 5000}, windows from recommendedWindowSize -- are built with BOTH parameters at
    // compile time (the window loop unrolled, 42 registers instead of 61 in k_sketch_fast); any other window takes the
    // run-time form of its k.
#define FA_KW_CELLS(X) X(14, 12) X(14, 37) X(14, 50) X(16, 13) X(16, 24) X(16, 40) X(21, 15) X(21, 25)
    // fused with the per-fragment sketch (k_query_fused, one of those cells): fragments whose records fit QF_CAP with room to
    // spare (a denser one voids the pass).  Tiles that touch a byte outside ACGT are sketched by k_sketch_tiles<0, true> into the
    // staging arrays FIRST (a launch whose other workgroups exit at once, and which carries the zeroing workgroups of the pass);
    // the fused kernel takes their records from there.  The run-time-w forms of the fused kernel do not fit the registers of seven waves per
    // SIMD -- a few words would go to scratch memory, which the runtime then keeps per stream for good -- and are not built.
    const bool fuse_on = knob::query_fused() != 0;
    const bool may_fuse = fuse && fuse_on && (int64_t)5 * P.fragment_length / (P.window_size + 1) <= QF_CAP;
    auto launch_fast = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(ntiles + extra), dim3(SK_THREADS), flds, st, a);
      extra = 0; a.clear.count = 0; a.clear.stamp = nullptr;
    };
    bool served = false;
#define FA_TRY_CELL(K, W)                                                                                                        \
    if (!served && P.kmer_size == K && P.window_size == W) {                                                                      \
      served = true;                                                                                                              \
      if (may_fuse) {                                                                                                             \
        QuerySketchArgs qa = *fuse;                                                                                               \
        qa.exc_tiles = store.n_exc > 0 ? 1 : 0;                                                                                   \
        if (store.n_exc > 0) launch(k_sketch_tiles<0, true>);                                                                     \
        const size_t qlds = flds + (size_t)QF_CAP * 4;                                                                            \
        hipLaunchKernelGGL((k_query_fused<K, W>), dim3((unsigned)F + extra), dim3(SK_THREADS), qlds, st, a, qa, (int)F);            \
        FA_HIP(hipGetLastError());                                                                                                \
        return true;                                                                                                              \
      }                                                                                                                           \
      launch_fast(k_sketch_fast<K, W>);                                                                                           \
    }
    FA_KW_CELLS(FA_TRY_CELL)
#undef FA_TRY_CELL
#undef FA_KW_CELLS
    if (served) {}
    else if (P.kmer_size == 16) launch_fast(k_sketch_fast<16, 0>);
    else if (P.kmer_size == 14) launch_fast(k_sketch_fast<14, 0>);
    else if (P.kmer_size == 21) launch_fast(k_sketch_fast<21, 0>);
    else launch_fast(k_sketch_fast<0, 0>);
  } else if (!a.protein) { if (P.kmer_size == 16) launch(k_sketch_tiles<16, false>); else launch(k_sketch_tiles<0, false>); }
  if (a.protein || store.n_exc > 0) launch(k_sketch_tiles<0, true>);
  FA_HIP(hipGetLastError());
  return false;
}

// rocPRIM directly (device-wide scan / radix sort / run-length encode; sizes are size_t)
static void exclusive_sum_i32(DevBuf<unsigned char> &temp, const int32_t *in, int32_t *out, size_t n, hipStream_t st) {
  with_temp(temp, [&](void *t, size_t &bytes) { return rocprim::exclusive_scan(t, bytes, in, out, (int32_t)0, n, rocprim::plus<int32_t>(), st); });
}

// ------------------------------------------------------------------------------------------------------------
// fa_sketch: reference genomes being collected (skch::Sketch + pyfastani's counters)
// ------------------------------------------------------------------------------------------------------------
// the minimizer records of a sketch: three parallel device arrays that grow, fill and empty together
struct RecArrays {
  DevBuf<uint32_t> hash;
  DevBuf<int32_t> seq, wpos;
  // room for n records, the first `keep` of them preserved
  void reserve(size_t n, size_t keep, hipStream_t st) { hash.ensure(n, true, st, keep); seq.ensure(n, true, st, keep); wpos.ensure(n, true, st, keep); }
  // n records from host (hipMemcpyHostToDevice) or device memory replace the content
  void load(const uint32_t *h, const int32_t *s, const int32_t *w, size_t n, hipMemcpyKind kind, hipStream_t st) {
    hash.ensure(n); seq.ensure(n); wpos.ensure(n);
    copy(hash.p, seq.p, wpos.p, h, s, w, n, kind, st);
  }
  // the first n records to host (hipMemcpyDeviceToHost) or device memory
  void store(uint32_t *h, int32_t *s, int32_t *w, size_t n, hipMemcpyKind kind, hipStream_t st) const { copy(h, s, w, hash.p, seq.p, wpos.p, n, kind, st); }
  static void copy(uint32_t *dh, int32_t *ds, int32_t *dw, const uint32_t *h, const int32_t *s, const int32_t *w, size_t n, hipMemcpyKind kind, hipStream_t st) {
    if (!n) return;
    FA_HIP(hipMemcpyAsync(dh, h, n * sizeof(uint32_t), kind, st));
    FA_HIP(hipMemcpyAsync(ds, s, n * sizeof(int32_t), kind, st));
    FA_HIP(hipMemcpyAsync(dw, w, n * sizeof(int32_t), kind, st));
  }
};

struct fa_sketch {
  fa_params P;
  int device = -1;
  hipStream_t stream = nullptr;
  hipStream_t up_stream = nullptr;        // uploads of a flush (the next chunk's sequence while this one is hashed)
  HostStore pending;                      // packed contigs not yet sketched
  RefBook book;                           // the genomes' counters, and the contig id of each pending sequence (fa_ingest.h)
  RecArrays rec;
  int64_t nrec = 0;
  SketchWork work;
  std::mutex mtx;

  void reset_data() {
    pending.clear(); pending.protein = P.alphabet_size != 4;
    book.reset(); nrec = 0;
  }

  // sketch every pending contig on the device and append the records
  void flush() {
    if (pending.seq_off.empty()) return;
    require_device();
    bind_device(device);
    if (!stream) FA_HIP(hipStreamCreate(&stream));
    StageTrace tr("sketch flush");
    // the packed sequence goes up chunk by chunk on a stream of its own: the copy of chunk c + 1 (a staged copy from pageable
    // memory: the host thread is inside it) runs while the device hashes chunk c -- 25-50 ms of a thousand genomes' 90-110
    if (!up_stream) FA_HIP(hipStreamCreate(&up_stream));
    DevStore store;
    store.begin(pending, stream);
    const int64_t nseq_all = (int64_t)pending.seq_off.size();
    // staging is 8 B per k-mer position; a chunk takes an eighth of the free HBM at most, between 96 M positions (768 MiB) and
    // 512 M (4 GiB: a thousand genomes are ten chunks, not fifty-two with two synchronisations each -- and not two chunks whose
    // 34 GB of staging a fresh process has to map first)
    size_t hbm_free = 0, hbm_total = 0;
    if (hipMemGetInfo(&hbm_free, &hbm_total) != hipSuccess) { (void)hipGetLastError(); hbm_free = 0; }
    const int64_t chunk_positions = std::max<int64_t>(96LL << 20, std::min<int64_t>((int64_t)(hbm_free / 8 / 8), 512LL << 20));
    // the records are appended chunk by chunk: reserve for all of them once (2 / (w + 1) of the positions are minimizers, a
    // quarter of headroom; `ensure(keep)` below still grows the arrays if a sequence is denser) instead of regrowing -- and
    // copying -- them a dozen times
    {
      int64_t positions_all = 0;
      for (int64_t q = 0; q < nseq_all; q++) positions_all += pending.seq_len[q];
      const double per_pos = P.alphabet_size == 4 ? 2.0 / (P.window_size + 1) : 1.0;
      const size_t expect = (size_t)nrec + (size_t)((double)positions_all * std::min(1.0, per_pos * 1.25)) + 1024;
      rec.reserve(expect, (size_t)nrec, stream);
    }
    // chunk boundaries first (the copy of the next chunk is issued while this one is hashed)
    std::vector<int64_t> cuts{0};
    for (int64_t q = 0, positions = 0; q < nseq_all; q++) {
      if (q > cuts.back() && positions + pending.seq_len[q] > chunk_positions) { cuts.push_back(q); positions = 0; }
      positions += pending.seq_len[q];
    }
    cuts.push_back(nseq_all);
    auto base_of = [&](int64_t q) { return q < nseq_all ? pending.seq_off[(size_t)q] : pending.total; };
    std::vector<hipEvent_t> sent(cuts.size() - 1, nullptr);
    struct EventsGuard { std::vector<hipEvent_t> &v; ~EventsGuard() { for (hipEvent_t e : v) if (e) (void)hipEventDestroy(e); } } events_guard{sent};
    auto send = [&](size_t c) {
      store.upload_bases(pending, base_of(cuts[c]), base_of(cuts[c + 1]), up_stream);
      FA_HIP(hipEventCreateWithFlags(&sent[c], hipEventDisableTiming));
      FA_HIP(hipEventRecord(sent[c], up_stream));
    };
    FA_HIP(hipStreamSynchronize(stream));           // (the buffers of `begin` exist before the other stream writes them)
    send(0);
    tr.mark("upload", up_stream);
    DevBuf<int32_t> d_seq_tile_lo, d_drop, d_drop_off, d_seq_ids;
    for (size_t chunk = 0; chunk + 1 < cuts.size(); chunk++) {
      const int64_t s0 = cuts[chunk], s1 = cuts[chunk + 1];
      std::vector<Tile> tiles;
      std::vector<int32_t> seq_tile_lo, seq_ids;
      // (tiles whose positions + halo are whole hashing trips: k1_tile_len)
      const int tile_len = k1_tile_len(P.window_size);
      // (five million tiles for a thousand genomes: counted first, then filled by the host pool -- 91 ms of one thread before)
      int64_t tile_total = 0;
      for (int64_t q = s0; q < s1; q++) {
        seq_tile_lo.push_back((int32_t)tile_total);
        tile_total += tile_count(pending.seq_len[q], P.kmer_size, tile_len);
        seq_ids.push_back(book.pending_contig[q]);
      }
      seq_tile_lo.push_back((int32_t)tile_total);
      FA_REQUIRE(tile_total < (1LL << 31) - 1, FA_ERR_UNSUPPORTED, "too many tiles in one sketch chunk");
      tiles.resize((size_t)tile_total);
      {
        const int64_t nq = s1 - s0, per = std::max<int64_t>(1, nq / 512);       // (a few hundred tasks at most)
        HostPool::get().parallel_for((size_t)((nq + per - 1) / per), [&](size_t t) {
          for (int64_t q = s0 + (int64_t)t * per; q < std::min(s1, s0 + ((int64_t)t + 1) * per); q++)
            make_tiles_at(tiles.data() + seq_tile_lo[(size_t)(q - s0)], pending, pending.seq_off[q], pending.seq_len[q], (int)(q - s0), P.kmer_size, P.window_size, tile_len);
        });
      }
      const int nseq = (int)(s1 - s0), ntiles = (int)tiles.size();
      tr.mark("host_tiles", stream);
      if (ntiles > 0) {
        work.tiles.upload(tiles, stream);
        work.stage_hash.ensure((size_t)ntiles * TILE);
        work.stage_wpos.ensure((size_t)ntiles * TILE);
        work.tile_count.ensure(ntiles + 1);
        work.tile_off.ensure(ntiles + 1);
        FA_HIP(hipMemsetAsync(work.tile_count.p + ntiles, 0, sizeof(int32_t), stream));
        tr.mark("alloc_tiles", stream);
        FA_HIP(hipStreamWaitEvent(stream, sent[chunk], 0));
        launch_sketch_tiles(P, store.view(), work.tiles.p, ntiles, work.stage_hash.p, work.stage_wpos.p, work.tile_count.p, stream);
        if (chunk + 2 < cuts.size()) send(chunk + 1);          // (behind the launch: the host copies while the device hashes)
        tr.mark("k_sketch", stream);
        d_seq_tile_lo.upload(seq_tile_lo, stream);
        d_seq_ids.upload(seq_ids, stream);
        d_drop.ensure(nseq + 1);
        d_drop_off.ensure(nseq + 1);
        FA_HIP(hipMemsetAsync(d_drop.p + nseq, 0, sizeof(int32_t), stream));
        hipLaunchKernelGGL(k_suppress_runs, dim3(ceil_div(nseq, 128)), dim3(128), 0, stream, d_seq_tile_lo.p, nseq,
                           work.tile_count.p, work.stage_hash.p, work.stage_wpos.p, d_drop.p);
        exclusive_sum_i32(work.cub_temp, work.tile_count.p, work.tile_off.p, ntiles + 1, stream);
        exclusive_sum_i32(work.cub_temp, d_drop.p, d_drop_off.p, nseq + 1, stream);
        int32_t total = 0, dropped = 0;
        FA_HIP(hipMemcpyAsync(&total, work.tile_off.p + ntiles, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        FA_HIP(hipMemcpyAsync(&dropped, d_drop_off.p + nseq, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        FA_HIP(hipStreamSynchronize(stream));
        const int64_t nout = (int64_t)total - dropped;
        tr.mark("scan", stream);
        rec.reserve((size_t)(nrec + nout), (size_t)nrec, stream);
        tr.mark("grow", stream);
        hipLaunchKernelGGL(k_compact_records, dim3(ntiles), dim3(256), 0, stream, work.tiles.p, work.tile_count.p,
                           work.tile_off.p, d_seq_tile_lo.p, d_drop.p, d_drop_off.p, work.stage_hash.p, work.stage_wpos.p,
                           d_seq_ids.p, nrec, rec.hash.p, rec.seq.p, rec.wpos.p);
        FA_HIP(hipGetLastError());
        FA_HIP(hipStreamSynchronize(stream));
        tr.mark("compact", stream);
        nrec += nout;
      } else if (chunk + 2 < cuts.size()) send(chunk + 1);
    }
    FA_HIP(hipStreamSynchronize(up_stream));
    pending.clear();
    pending.protein = P.alphabet_size != 4;
    book.pending_contig.clear();
  }
};

// ------------------------------------------------------------------------------------------------------------
// fa_genomes: packed query genomes resident in HBM, cut into fragments and tiles
// ------------------------------------------------------------------------------------------------------------
// Pinned host staging memory (grows, never shrinks; one per workspace / upload)
struct PinnedBuf {
  unsigned char *p = nullptr;
  size_t cap = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf &operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  void ensure(size_t n) {
    if (n <= cap) return;
    if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
    const size_t ncap = std::max(n, cap * 2);
    FA_HIP(hipHostMalloc((void **)&p, ncap, hipHostMallocDefault));
    cap = ncap;
  }
};

// Everything the kernels read of a batch sits in ONE device allocation, filled by ONE host-to-device copy from a staging
// image of the same layout (BatchLayout, fa_ingest.h).  Only the exception lists (rare: N runs, IUPAC codes) are separate.
struct fa_genomes {
  fa_params P;
  DevBuf<unsigned char> blob;
  DevBuf<int64_t> exc_pos;
  DevBuf<uint8_t> exc_val;
  StoreView store;                          // pointers into blob / the exception buffers
  const Tile *tiles = nullptr;
  const int32_t *d_frag_tile_lo = nullptr, *d_frag_query = nullptr, *d_frag_qseq = nullptr, *d_total_frag = nullptr;
  int32_t n_genomes = 0;
  std::vector<int64_t> genome_frag_lo;      // [n_genomes + 1] fragment range of each genome
  std::vector<int32_t> frag_tile_lo;        // [F + 1]
  std::vector<int64_t> contig_frag_lo;      // first fragment of every contig that holds fragments (ascending)
  std::vector<uint64_t> total_fragments, total_length;
  std::vector<int32_t> n_short;
  int64_t F = 0, ntiles = 0;
  uint64_t total_bases = 0;                 // bases inside fragments
  std::vector<unsigned char, NoInitAlloc<unsigned char>> host_image;   // staging image when no pinned buffer is supplied (every byte of it is written: no zero fill)
  PinnedBuf pin_image;                      // staging image of a batch that is refilled (fa_genomes_reload_fasta)
  hipStream_t up_stream = nullptr;          // FASTA uploads run on the batch's own stream
  ~fa_genomes() { if (up_stream) (void)hipStreamDestroy(up_stream); }
  fa_genomes() = default;
  // a failed refill leaves an empty (but valid) batch
  void reset_empty() {
    n_genomes = 0; F = 0; ntiles = 0;
    genome_frag_lo.assign(1, 0); total_fragments.clear(); total_length.clear(); n_short.clear();
  }
  uint64_t serial = 0;                      // a new number for every upload (caches keyed on a batch compare this, not its address)
};
static std::atomic<uint64_t> g_batch_serial{0};

// The hand-over of a pass (publish_pass, fa_map.hip.h): copies the status block -- and, for a one-query call whose rows go to the host, the rows --
// into pinned host memory and then releases the pass number.  The host polls that word instead of waiting for a
// device-to-host copy and a stream synchronisation, which together return tens of microseconds after the GPU is done
// (more on a slow host: the step time of the bench varied by 0.09 ms between boxes on that account).
static PublishArgs publish_args(PassStatus *dev, PassStatus *host_mapped, uint32_t seq, const fa_cgi_row *rows_dev, fa_cgi_row *rows_host, int64_t cap) {
  PublishArgs p;
  p.status_dev = (uint32_t *)dev; p.status_host = (uint32_t *)host_mapped;
  p.words = (int32_t)(offsetof(PassStatus, seq) / 4); p.seq_word = p.words; p.seq = seq;
  p.stamp = dev->stamp; p.total_rows = &dev->total_rows;
  p.rows_dev = rows_dev; p.rows_host = rows_host; p.cap = cap;
  return p;
}
// host side of k_publish_status: polls for FA_SPIN_US microseconds (default 20 000), then sleeps on the stream
static void wait_published(const PassStatus *h, uint32_t seq, hipStream_t st) {
  if (spin_for_seq(&h->seq, seq, knob::spin_us())) return;
  FA_HIP(hipStreamSynchronize(st));
  FA_REQUIRE(__atomic_load_n(&h->seq, __ATOMIC_ACQUIRE) == seq, FA_ERR_INTERNAL, "the status of the pass was not published");
}

// The slots of Workspace::last_ms (fa_mapper_last_timings), laid out as include/fastani_hip.h documents: [MS_STAGE + 0..3] sketch,
// lookup + L1, L2, CGI ms; [MS_HOST + 0..2] the host-side split of fa_mapper_query; also [MS_L1_SORTED] [MS_L1_MERGED] (FA_L1_STATS
// samples) and [MS_L1_OFF_FAST] (fragments that left k_l1's fast form)
enum TimingSlot : int { MS_STAGE = 0, MS_TOTAL = 4, MS_RECORDS, MS_LOCI, MS_EVENTS, MS_WIDE, MS_REPEATS, MS_HOST = 10, MS_CALL = 13,
                        MS_L2_EVENTS = 16, MS_FUSED, MS_UNFUSED, MS_ORDERED, MS_L1_SORTED, MS_L1_MERGED, MS_L1_OFF_FAST, MS_TILE_LEN, MS_SLOTS };
static_assert(MS_REPEATS == 9 && MS_ORDERED == 19 && MS_TILE_LEN == 23 && MS_SLOTS == 24, "the layout of fa_mapper_last_timings is ABI");

// The way of the mapping records to the host: two buffers of `records` fa_hit_mapping in HBM, two in pinned host memory and an
// event each.  k_map_write fills HBM buffer w & 1 with window w of a pass (fa_mapstream.h), an asynchronous copy takes it to
// pinned buffer w & 1, and while the host consumes that the device works on window w + 1.  Their size is the mapper's
// (fa_mapper_set_mapping_stage), not the table's; allocated by the first call that wants mappings on the host.
struct MapStage {
  fa_hit_mapping *dev[2] = {nullptr, nullptr}, *pin[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  int64_t records = 0;
  MapStage() = default;
  MapStage(const MapStage &) = delete;
  MapStage &operator=(const MapStage &) = delete;
  ~MapStage() {
    release();
    for (auto &e : ev) if (e) (void)hipEventDestroy(e);
  }
  void release() {
    for (int i = 0; i < 2; i++) {
      if (dev[i]) (void)hipFree(dev[i]);
      if (pin[i]) (void)hipHostFree(pin[i]);
      dev[i] = pin[i] = nullptr;
    }
    records = 0;
  }
  // (the caller's stream is idle: a query call owns its workspace, and every call drains its windows before it returns)
  void resize(int64_t n) {
    if (n == records) return;
    release();
    for (int i = 0; i < 2; i++) {
      FA_HIP(hipMalloc((void **)&dev[i], (size_t)n * sizeof(fa_hit_mapping)));
      FA_HIP(hipHostMalloc((void **)&pin[i], (size_t)n * sizeof(fa_hit_mapping), hipHostMallocDefault));
      if (!ev[i]) FA_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
    }
    records = n;
  }
  size_t bytes() const { return dev[0] ? 2 * (size_t)records * sizeof(fa_hit_mapping) : 0; }
};

static fa_rules default_rules() { fa_rules r; r.l2_confidence = kConfidence; r.slide_end = 0; r.cgi_ties = 0; return r; }
static bool same_rules(const fa_rules &a, const fa_rules &b) {
  return a.l2_confidence == b.l2_confidence && a.slide_end == b.slide_end && a.cgi_ties == b.cgi_ties;
}

// Everything one query call owns: its stream, every intermediate of the pipeline, its status block and timing events.
struct Workspace {
  bool in_use = false;
  hipStream_t stream = nullptr;
  SketchWork sk;
  DevBuf<uint32_t> q_hash, q_off, q_cnt, n_seeds, ovf_off, ovf_buf;
  DevBuf<PassStatus> status;
  PassStatus *h_status = nullptr;     // pinned, written by k_publish_status
  uint32_t seq = 0;                   // passes published on this workspace
  DevBuf<int32_t> q_size, l_frag, l_seq, l_start, l_end, l_group, l_shared, l_pos, row_count, row_flag, row_off;
  DevBuf<int32_t> l_beg, l_end0, l_last, l_ndrop, l_rfirst, l_rlast, l_rpart;
  DevBuf<uint32_t> l_nev, l_ioff, f_loci_lo, f_loci_n;
  DevBuf<unsigned char> items;
  DevBuf<uint8_t> l_redo, big_state;
  DevBuf<uint32_t> scan_hist, scan_order;   // k_l2_scan's loci by stream length: class counts + cursors, the order
  // workgroup order of k_l2_events for passes of several genomes (L2Args::frag_order), cached while the same part repeats
  DevBuf<int32_t> frag_order;
  PinnedBuf pin_order;
  uint64_t order_batch = 0;            // fa_genomes::serial of the batch the cached order was built for
  int64_t order_f0 = -1, order_f1 = -1;
  uint32_t order_len = 0;
  DevBuf<unsigned long long> group_best, bins;
  DevBuf<float> row_ident;
  DevBuf<fa_cgi_row> rows_dev;
  // only on workspaces that served a call for the mappings behind the rows (MapSink): the winner table parallel to `bins`,
  // the chunk counts / offsets of the compaction, and the stage through which the records reach the host
  DevBuf<MapWinner> winners;
  DevBuf<int32_t> map_chunk_count;
  DevBuf<int64_t> map_chunk_off;
  MapStage map_stage;
  // LUT pointers captured for the call (the mapper may publish larger tables while this call is in flight)
  const int32_t *lut_min_hits = nullptr, *lut_pass = nullptr;
  const float *lut_ident = nullptr;
  // the mapper's rules as they stood when the call started (run_query): every pass of the call follows them.  `own_pass`: the
  // pass table of a call whose interval the mapper has left since (fa_mapper_set_rules while the call was in flight)
  fa_rules rules = default_rules();
  DevBuf<int32_t> own_pass;
  // last-pass bookkeeping for the debug getters
  int64_t last_F = 0;
  uint32_t last_loci = 0;             // loci of the last accepted part (all regions)
  uint32_t loci_n = 1, loci_shift = 0;                    // regions of the locus numbering of the part in flight / last accepted
  uint32_t last_region_count[LOCI_REGIONS] = {0};         // live loci per region of the last accepted part
  uint64_t last_items = 0;
  const fa_genomes *last_genomes = nullptr;
  float last_ms[MS_SLOTS] = {0};
  hipEvent_t ev[6] = {nullptr};
  int64_t pass_F = 0;                 // fragments of the last pass
  // the kernel forms of a part (fa_mapper_debug_spec): those of the part in flight, and those of the last part accepted in the
  // last call (cleared when a call starts)
  Forms forms, last_forms;
  // the one-query-at-a-time call (fa_mapper_query) recycles its batch object -- no device allocation per call -- and
  // builds the upload image in pinned memory; its rows come back through a pinned block too
  std::unique_ptr<fa_genomes> query_batch;
  PinnedBuf pin_image, pin_rows;
  ~Workspace() {
    for (auto &e : ev) if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    if (h_status) (void)hipHostFree(h_status);
  }
};

// ------------------------------------------------------------------------------------------------------------
// fa_mapper: the indexed reference + the workspace of the query pipeline
// ------------------------------------------------------------------------------------------------------------
struct fa_mapper {
  fa_params P;
  int device = -1;
  hipStream_t stream = nullptr;
  std::mutex mtx;
  // reference records and index (see fa_map.hip.h for the layout)
  DevBuf<uint32_t> rec_hash, uniq_hash, uniq_off, pos_ridx;
  DevBuf<uint4> table;
  DevBuf<int32_t> rec_seq, rec_wpos, rec_prev, rec_fwd, rec_bwd, contig_rec, contig_genome, contig_bin, genome_bin;
  DevBuf<uint8_t> rec_flags;
  DevBuf<uint2> rec_hg;           // (hash, packed window geometry + flags) for k_l2_events (empty when cmw >= 8191)
  DevBuf<uint16_t> rec_prev16;
  DevBuf<uint32_t> rec_gpos, wrap_rec;   // padded global coordinate of every record (low word) + its 2^32 boundaries, for k_l1
  int32_t n_wraps = 0, gpos_bits = 32;
  bool packed_geo = false;
  // k_l2_events reads the packed record layout (rec_hg, rec_prev16) when the index has one; FA_NO_PACKED_GEO=1 takes the
  // plain arrays on any index (the tests reach the unpacked form on small indices that way).  Asked once per part (QueryPass::ev_packed)
  bool events_packed() const { return packed_geo && !knob::no_packed_geo(); }
  int64_t N = 0, U = 0;
  int32_t C = 0, G = 0, table_bits = 4, freq_threshold = INT_MAX, total_bins = 0;
  std::vector<uint64_t> lengths;
  std::vector<int32_t> seqs_by_file;
  int32_t cmw = 0, qcap = 1;
  // the open readings of the arithmetic this mapper follows (fa_mapper_set_rules); stats.ci mirrors rules.l2_confidence
  fa_rules rules = default_rules();
  // LUTs
  StatTables stats;
  DevBuf<int32_t> d_min_hits, d_pass;
  DevBuf<float> d_ident;
  // data-dependent sizes speculated from earlier passes (see run_query_pass); shared by all workspaces, guarded by mtx
  Spec spec;
  // Queries are re-entrant (_fastani.pyx:1158-1161): every call takes one of NWS workspaces -- its own stream and every
  // intermediate of the pipeline -- so calls from different host threads overlap on the device (their phases interleave,
  // which is worth ~27 % of throughput over strictly serial calls).  `mtx` guards the pool, the speculation record and
  // the LUTs; the index itself is read-only.
  static constexpr int NWS = 4;
  Workspace ws[NWS];
  std::condition_variable ws_free;
  int last_ws = 0;                    // workspace of the most recent call (stage getters, timings)
  // records per stage buffer of the streamed mapping output (MapStage; fa_mapper_set_mapping_stage, default FA_MAP_STAGE_MB),
  // and the workspace of the most recent call that asked for mappings (fa_mapper_mapping_memory)
  int64_t map_stage = std::max<int64_t>(1, (int64_t)knob::map_stage_mb() * (1024 * 1024 / (int64_t)sizeof(fa_hit_mapping)));
  int last_map_ws = -1;
  bool stage_events = false;          // fa_mapper_set_stage_events
  std::vector<DevBuf<int32_t>> retired_i32;   // LUT generations still referenced by calls in flight
  std::vector<DevBuf<float>> retired_f32;

  IndexView view() const {
    IndexView v;
    v.rec_hash = rec_hash.p; v.rec_seq = rec_seq.p; v.rec_wpos = rec_wpos.p; v.rec_prev = rec_prev.p; v.rec_fwd = rec_fwd.p; v.rec_bwd = rec_bwd.p; v.rec_flags = rec_flags.p;
    v.rec_hg = packed_geo ? rec_hg.p : nullptr; v.rec_prev16 = packed_geo ? rec_prev16.p : nullptr; v.rec_gpos = rec_gpos.p; v.wrap_rec = wrap_rec.p; v.n_wraps = n_wraps; v.gpos_bits = gpos_bits;
    v.uniq_hash = uniq_hash.p; v.uniq_off = uniq_off.p; v.pos_ridx = pos_ridx.p; v.table = table.p;
    v.contig_rec = contig_rec.p; v.contig_genome = contig_genome.p; v.contig_bin = contig_bin.p; v.genome_bin = genome_bin.p;
    v.N = N; v.U = U; v.C = C; v.G = G; v.table_bits = table_bits; v.freq_threshold = freq_threshold; v.total_bins = total_bins;
    return v;
  }
};

__global__ void k_contig_bins(const int32_t *contig_rec, const int32_t *rec_wpos, int C, int bin_len, int32_t *nbins) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > C) return;
  int n = 0;
  if (c < C) {
    int lo = contig_rec[c], hi = contig_rec[c + 1];
    if (hi > lo) n = rec_wpos[hi - 1] / bin_len + 1;
  }
  nbins[c] = n;
}

// Sketch_t::computeFreqHist on the device: the frequency threshold of U position lists of the lengths `counts` (a device
// array), INT_MAX when nothing is ignored.  The one copy of the walk: build_index and fa_sketch_frequency both call it.
static int frequency_threshold(const uint32_t *counts, int64_t U, DevBuf<unsigned char> &temp, hipStream_t st) {
  int threshold = INT_MAX;
  DevBuf<uint32_t> counts_sorted;
  // frequency threshold (computeFreqHist): walk the distinct list lengths from the most frequent down
  int64_t to_ignore = (int64_t)((float)U * 0.001f / 100);
  int64_t M = std::min<int64_t>(U, to_ignore + 1);
  // the M largest list lengths, in descending order: from a histogram of the short lists plus the long ones verbatim
  // (k_length_histogram); only an index with more than 65 536 lists of 4 096 positions and more sorts all lengths instead
  std::vector<uint32_t> top;
  top.reserve((size_t)M);
  {
    // (FA_FREQ_OVER_CAP: the tests shrink the room for long lists -- 1 = none fits -- so that the sort is exercised too)
    const uint32_t OVER_CAP = (uint32_t)knob::freq_over_cap();
    DevBuf<unsigned long long> d_hist;
    DevBuf<uint32_t> d_over;
    d_hist.ensure(FREQ_BINS + 1); d_over.ensure(OVER_CAP);
    FA_HIP(hipMemsetAsync(d_hist.p, 0, (FREQ_BINS + 1) * sizeof(unsigned long long), st));
    uint32_t *d_over_n = (uint32_t *)(d_hist.p + FREQ_BINS);
    hipLaunchKernelGGL(k_length_histogram, dim3((unsigned)std::min<int64_t>(ceil_div(U, 256), 4096)), dim3(256), 0, st, counts, U, d_hist.p,
                       d_over.p, OVER_CAP, d_over_n);
    std::vector<unsigned long long> h_hist(FREQ_BINS + 1);
    d_hist.download(h_hist.data(), FREQ_BINS + 1, st);
    FA_HIP(hipStreamSynchronize(st));
    const uint32_t n_over = (uint32_t)(h_hist[FREQ_BINS] & 0xFFFFFFFFu);
    if (n_over < OVER_CAP || n_over == 0) {
      std::vector<uint32_t> h_over(n_over);
      if (n_over) { d_over.download(h_over.data(), n_over, st); FA_HIP(hipStreamSynchronize(st)); }
      std::sort(h_over.begin(), h_over.end(), std::greater<uint32_t>());
      for (uint32_t i = 0; i < n_over && (int64_t)top.size() < M; i++) top.push_back(h_over[i]);
      for (int b = FREQ_BINS - 1; b >= 0 && (int64_t)top.size() < M; b--)
        for (unsigned long long c = h_hist[(size_t)b]; c > 0 && (int64_t)top.size() < M; c--) top.push_back((uint32_t)b);
    } else {
      counts_sorted.ensure((size_t)U);
      with_temp(temp, [&](void *t, size_t &bytes) {
        return rocprim::radix_sort_keys_desc(t, bytes, counts, counts_sorted.p, (size_t)U, 0u, 32u, st);
      });
      top.resize((size_t)M);
      counts_sorted.download(top.data(), (size_t)M, st);
      FA_HIP(hipStreamSynchronize(st));
    }
  }
  FA_REQUIRE((int64_t)top.size() == M, FA_ERR_INTERNAL, "list-length histogram does not add up");
  for (int64_t i = 0; i < M;) {
    int64_t j = i;
    while (j < M && top[j] == top[i]) j++;
    if (j == M && M < U) break;   // the run continues past the prefix: sum would exceed to_ignore
    if (j < to_ignore) { threshold = (int)top[i]; i = j; }
    else if (j == to_ignore) { threshold = (int)top[i]; break; }
    else break;
  }
  return threshold;
}

// Sketch_t::index() + computeFreqHist() on the device
static void build_index(fa_mapper &m) {
  hipStream_t st = m.stream;
  const int64_t N = m.N;
  // record numbers are 32-bit throughout the mapping kernels (a seed hit IS a record number): 2^31 minimizers, about 5 000
  // genomes of 5 Mb, per index -- beyond that shard the references (sharding.build_ref_sharded_mapper)
  // (k_window_links adds up to a fragment's windows + 2 to a record number in 32-bit arithmetic: that much headroom below 2^31)
  FA_REQUIRE(N < (1LL << 31) - 1 - (int64_t)std::max(0, m.P.fragment_length) - 64, FA_ERR_UNSUPPORTED, "more than 2^31 minimizers in one index (shard the references)");
  m.C = m.seqs_by_file.empty() ? 0 : m.seqs_by_file.back();
  m.G = (int32_t)m.seqs_by_file.size();
  // minimizer windows per fragment.  When it is <= 0 no fragment holds a window, query sketches are empty and L2 never
  // runs (the degenerate (k=21, fragment 1000) cell); the window links are then built for 1 and never read
  m.cmw = std::max(1, m.P.fragment_length - (m.P.window_size - 1) - (m.P.kmer_size - 1));
  m.qcap = std::max(1, m.P.fragment_length - m.P.kmer_size + 1 - (m.P.window_size - 1));
  const int bin_len = m.P.fragment_length - 20;
  DevBuf<unsigned char> temp;
  StageTrace tr("build_index");
  // contig tables
  std::vector<int32_t> cg((size_t)m.C + 1, 0);
  {
    int g = 0;
    for (int c = 0; c < m.C; c++) {
      while (g < m.G && m.seqs_by_file[g] <= c) g++;
      cg[c] = g;
    }
  }
  m.contig_genome.upload(cg, st);
  m.contig_rec.ensure((size_t)m.C + 2);
  hipLaunchKernelGGL(k_contig_ranges, dim3(ceil_div(m.C + 1, 256)), dim3(256), 0, st, m.rec_seq.p, N, m.C, m.contig_rec.p);
  DevBuf<int32_t> nbins;
  nbins.ensure((size_t)m.C + 2);
  m.contig_bin.ensure((size_t)m.C + 2);
  hipLaunchKernelGGL(k_contig_bins, dim3(ceil_div(m.C + 1, 256)), dim3(256), 0, st, m.contig_rec.p, m.rec_wpos.p, m.C,
                     bin_len > 0 ? bin_len : 1, nbins.p);
  exclusive_sum_i32(temp, nbins.p, m.contig_bin.p, m.C + 1, st);
  std::vector<int32_t> cb((size_t)m.C + 1);
  m.contig_bin.download(cb.data(), (size_t)m.C + 1, st);
  FA_HIP(hipStreamSynchronize(st));
  m.total_bins = cb[m.C];
  std::vector<int32_t> gb((size_t)m.G + 1);
  for (int g = 0; g <= m.G; g++) {
    int c = g == 0 ? 0 : m.seqs_by_file[g - 1];
    gb[g] = cb[std::min(c, m.C)];
  }
  m.genome_bin.upload(gb, st);
  tr.mark("contigs", st);

  // hash-grouped order (stable radix sort keeps record order inside a hash group)
  m.pos_ridx.ensure((size_t)N + 4);
  m.rec_prev.ensure((size_t)N + 4);
  m.rec_fwd.ensure((size_t)N + 4);
  m.rec_bwd.ensure((size_t)N + 4);
  m.rec_flags.ensure(((size_t)N + 7) / 4 * 4);
  FA_HIP(hipMemsetAsync(m.rec_flags.p, 0, ((size_t)N + 7) / 4 * 4, st));
  m.U = 0;
  m.freq_threshold = INT_MAX;
  if (N > 0) {
    DevBuf<uint32_t> iota, sorted_hash, counts, blk_lo;
    DevBuf<int32_t> num_runs;
    iota.ensure((size_t)N); sorted_hash.ensure((size_t)N); counts.ensure((size_t)N + 1); num_runs.ensure(1);
    tr.mark("alloc", st);
    hipLaunchKernelGGL(k_iota, dim3(ceil_div(N, 256)), dim3(256), 0, st, iota.p, N);
    with_temp(temp, [&](void *t, size_t &bytes) {
      return rocprim::radix_sort_pairs(t, bytes, m.rec_hash.p, sorted_hash.p, iota.p, m.pos_ridx.p, (size_t)N, 0u, 32u, st);
    });
    tr.mark("sort", st);
    m.uniq_hash.ensure((size_t)N + 1);
    with_temp(temp, [&](void *t, size_t &bytes) {
      return rocprim::run_length_encode(t, bytes, sorted_hash.p, (size_t)N, m.uniq_hash.p, counts.p, num_runs.p, st);
    });
    int32_t U = 0;
    num_runs.download(&U, 1, st);
    FA_HIP(hipStreamSynchronize(st));
    m.U = U;
    FA_HIP(hipMemsetAsync(counts.p + U, 0, sizeof(uint32_t), st));
    m.uniq_off.ensure((size_t)U + 2);
    with_temp(temp, [&](void *t, size_t &bytes) {
      return rocprim::exclusive_scan(t, bytes, counts.p, m.uniq_off.p, 0u, (size_t)U + 1, rocprim::plus<uint32_t>(), st);
    });
    tr.mark("rle_scan", st);
    m.freq_threshold = frequency_threshold(counts.p, (int64_t)U, temp, st);
    tr.mark("threshold", st);
    // lookup table at load factor <= 1/2
    m.table_bits = std::max(4, floor_log2(std::max(U, 1)) + 2);
    FA_REQUIRE(m.table_bits <= 31, FA_ERR_UNSUPPORTED, "too many distinct minimizers for the lookup table");
    m.table.ensure((size_t)1 << m.table_bits);
    tr.mark("table_alloc", st);
    FA_HIP(hipMemsetAsync(m.table.p, 0, ((size_t)1 << m.table_bits) * sizeof(uint4), st));
    tr.mark("table_clear", st);
    hipLaunchKernelGGL(k_build_table, dim3(ceil_div(U, 256)), dim3(256), 0, st, m.uniq_hash.p, m.uniq_off.p, (int64_t)U, m.table_bits, m.table.p);
    tr.mark("table", st);
    {
      // window links first (they write the flag bytes whole), then the same-hash links OR their bits in
      const int halo = (int)std::min<int64_t>(((int64_t)m.cmw + 2 + 63) / 64 * 64, WL_HALO_MAX);
      if (halo >= m.cmw + 2)
        hipLaunchKernelGGL(k_window_links<true>, dim3(ceil_div(N, WL_TILE)), dim3(WL_THREADS), (size_t)(WL_TILE + 2 * halo) * sizeof(int32_t), st, m.rec_seq.p,
                           m.rec_wpos.p, m.contig_rec.p, N, m.cmw, halo, m.rec_fwd.p, m.rec_bwd.p, m.rec_flags.p);
      else
        hipLaunchKernelGGL(k_window_links<false>, dim3(ceil_div(N, WL_TILE)), dim3(WL_THREADS), (size_t)(WL_TILE + 2 * halo) * sizeof(int32_t), st, m.rec_seq.p,
                           m.rec_wpos.p, m.contig_rec.p, N, m.cmw, halo, m.rec_fwd.p, m.rec_bwd.p, m.rec_flags.p);
      // (FA_LINK_BLOCK_BITS: the tests shrink the blocks so that a small index has blocks inside a contig AND straddling ones)
      const int shift = (int)knob::link_block_bits();
      const int64_t blocks = (N + ((int64_t)1 << shift) - 1) >> shift;
      blk_lo.ensure((size_t)blocks + 1);
      hipLaunchKernelGGL(k_block_contig, dim3(ceil_div(blocks, 256)), dim3(256), 0, st, m.rec_seq.p, m.contig_rec.p, N, shift, blk_lo.p);
      FA_HIP(hipMemsetAsync(m.rec_prev.p, 0xFF, (size_t)N * sizeof(int32_t), st));
      hipLaunchKernelGGL(k_link_duplicates, dim3(ceil_div(N, 256)), dim3(256), 0, st, sorted_hash.p, m.pos_ridx.p, N, m.rec_seq.p, m.rec_wpos.p,
                         m.contig_rec.p, blk_lo.p, shift, m.cmw, m.rec_prev.p, m.rec_flags.p);
    }
    tr.mark("links", st);
    {
      // padded global coordinate of every record (k_rec_gpos): spans of the contigs, their prefix sums, the low words
      DevBuf<unsigned long long> span, base;
      DevBuf<int32_t> d_wraps;
      span.ensure((size_t)m.C + 2); d_wraps.ensure(1);
      hipLaunchKernelGGL(k_contig_span, dim3(ceil_div(m.C + 1, 256)), dim3(256), 0, st, m.contig_rec.p, m.rec_wpos.p, m.C, m.P.fragment_length, span.p);
      // (the prefix sums on the host: a contig list is small next to the records, and a 64-bit device scan would be the one
      // kernel of the library that needs scratch memory, which the runtime keeps per stream for good)
      std::vector<unsigned long long> h_span((size_t)m.C + 1), h_base((size_t)m.C + 1);
      span.download(h_span.data(), (size_t)m.C + 1, st);
      FA_HIP(hipStreamSynchronize(st));
      unsigned long long run = 0;
      for (int c = 0; c <= m.C; c++) { h_base[(size_t)c] = run; run += h_span[(size_t)c]; }
      base.upload(h_base, st);
      m.rec_gpos.ensure((size_t)N + 4);
      m.wrap_rec.ensure(GPOS_MAX_WRAPS);
      // (FA_GPOS_BITS: the tests shrink the low word so that a small index crosses many of its boundaries)
      m.gpos_bits = (int)knob::gpos_bits();
      FA_REQUIRE(m.gpos_bits == 32 || (1LL << m.gpos_bits) > 2 * (int64_t)m.P.fragment_length, FA_ERR_INVALID, "FA_GPOS_BITS too small for the fragment length");
      hipLaunchKernelGGL(k_rec_gpos, dim3(ceil_div(N, 256)), dim3(256), 0, st, m.rec_seq.p, m.rec_wpos.p, base.p, N, m.gpos_bits, m.rec_gpos.p, m.wrap_rec.p, d_wraps.p);
      d_wraps.download(&m.n_wraps, 1, st);
      FA_HIP(hipStreamSynchronize(st));
      FA_REQUIRE(m.n_wraps <= GPOS_MAX_WRAPS, FA_ERR_UNSUPPORTED, m.gpos_bits == 32 ? "the index spans more than 2^40 bases (shard the references)"
                                                                                       : "FA_GPOS_BITS: more than 256 boundaries in this index");
    }
    m.packed_geo = m.cmw + 1 < (1 << GEO_BITS);
    if (m.packed_geo) {
      m.rec_hg.ensure((size_t)N + 4); m.rec_prev16.ensure((size_t)N + 4);
      hipLaunchKernelGGL(k_pack_geometry, dim3(ceil_div(N, 256)), dim3(256), 0, st, m.rec_hash.p, m.rec_prev.p, m.rec_fwd.p, m.rec_bwd.p, m.rec_flags.p, N,
                         m.rec_hg.p, m.rec_prev16.p);
    }
    FA_HIP(hipGetLastError());
    FA_HIP(hipStreamSynchronize(st));
    tr.mark("geometry", st);
  } else {
    m.table_bits = 4;
    m.table.ensure(16);
    FA_HIP(hipMemsetAsync(m.table.p, 0, 16 * sizeof(uint4), st));
    m.uniq_hash.ensure(2); m.uniq_off.ensure(2);
    m.rec_gpos.ensure(4); m.wrap_rec.ensure(GPOS_MAX_WRAPS); m.n_wraps = 0;
    FA_HIP(hipMemsetAsync(m.uniq_off.p, 0, 2 * sizeof(uint32_t), st));
    FA_HIP(hipStreamSynchronize(st));
  }
  m.stats.k = m.P.kmer_size;
  m.stats.pid = m.P.percentage_identity;
  m.stats.smax = -1;
}

// ------------------------------------------------------------------------------------------------------------
// query pipeline over the fragment range [f0, f1) of a resident batch
// ------------------------------------------------------------------------------------------------------------
// (Re)builds the LUTs for sketches up to smax.  Called with m.mtx held; calls in flight keep the tables they captured
// (older generations are retired, not freed), so the tables can grow while other workspaces are busy.
static void ensure_luts(fa_mapper &m, int smax) {
  if (m.stats.extend(std::max(smax, 1))) {
    if (m.d_min_hits.p) { m.retired_i32.push_back(std::move(m.d_min_hits)); m.retired_i32.push_back(std::move(m.d_pass)); m.retired_f32.push_back(std::move(m.d_ident)); }
    m.d_min_hits.upload(m.stats.min_hits, m.stream);
    m.d_pass.upload(m.stats.pass_shared, m.stream);
    m.d_ident.upload(m.stats.ident, m.stream);
    FA_HIP(hipStreamSynchronize(m.stream));
  }
}



// zero several device ranges with one launch (every DevBuf is at least 16-byte aligned; sizes are rounded up to 16 bytes:
// the buffers listed below are allocated with slack, and the cleared prefix of the status block is a multiple of 16 bytes
// -- asserted next to PassStatus -- so the rounding never reaches the stamps behind it)
struct ClearList {
  ClearArgs a;
  ClearList() { a.count = 0; a.stamp = nullptr; }
  void add(void *p, size_t bytes) {
    if (!bytes) return;
    FA_REQUIRE(a.count < (int)(sizeof(a.ptr) / sizeof(a.ptr[0])), FA_ERR_INTERNAL, "more ranges to clear than ClearArgs holds");
    a.ptr[a.count] = (uint4 *)p; a.n16[a.count] = (bytes + 15) / 16; a.count++;
  }
  void launch(hipStream_t st) {
    if (!a.count) return;
    uint64_t most = 0;
    for (int i = 0; i < a.count; i++) most = std::max(most, a.n16[i]);
    int blocks = (int)std::min<uint64_t>(2048, std::max<uint64_t>(1, (most + 255) / 256));
    hipLaunchKernelGGL(k_clear, dim3(blocks), dim3(256), 0, st, a);
    a.count = 0;
  }
};

// FA_DEBUG_SYNC=1: synchronise after every stage of a query pass and name the stage that failed
static void debug_sync(hipStream_t st, const char *stage) {
  if (!knob::debug_sync()) return;
  fprintf(stderr, "[fa] %s ...\n", stage);
  hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) throw Error(FA_ERR_NO_DEVICE, std::string("stage ") + stage + " failed: " + hipGetErrorString(e));
}

// fragments mapped per pass (bounds the workspace); FA_PASS_FRAGMENTS overrides it (tests force several passes)
static int64_t pass_fragments() { return (int64_t)knob::pass_fragments(); }

// Dynamic LDS of k_l2_events and k_l2_scan at a sketch bound (their tables hold cnt_slots = smax + 1 ranks) for the fragments
// of an index: what scan_occupancy asks the runtime about is what launch_l2_stage launches with.
struct L2Lds {
  int slots, ev_stage, scan_class_div;
  size_t events;
  L2Lds(const fa_params &P, int smax, bool wide) : slots(smax + 1) {
    const int per_window = std::max(1, 2 * P.fragment_length / (P.window_size + 1));
    // events of one locus staged in LDS per wave of k_l2_events (longer streams are stored directly): a stream holds
    // the records of about 2.6 windows twice, minus the first window -- 5.3 windows' worth at the longest in the bench;
    // the LDS this costs decides how many workgroups a CU holds (2048: 6, 1408: 7; 0.41 vs 0.38 ms for the L2 stage)
    ev_stage = std::min(2048, std::max(512, (per_window * 11 / 2 + 127) & ~127));
    events = ev_sketch_bytes(slots) + (size_t)ev_stage * (wide ? 4 : 2) * (EV_THREADS / 64) + 16;
    // classes of k_l2_order's counting sort: the longest streams hold the records of ~2.6 windows twice (see ev_stage), so six
    // windows' worth of events over the classes
    scan_class_div = std::max(8, (per_window * 6 / SCAN_CLASSES + 7) & ~7);
  }
  // k_l2_scan with `lanes` loci per workgroup and `bytes` of state per rank (1: the fast pass, 2: the wide-state redo pass)
  size_t scan(int lanes, int bytes) const { return ((size_t)(slots + 1) * lanes * bytes + 15) / 16 * 16; }
};

// Where a call wants the mappings behind its rows; `on` = false: it does not, and the pass launches and allocates nothing
// for them.  Passes append: `base` records are in place.  `count` learns the number of records, also when they do not fit.
// The destination is one of: `dev`, the caller's device buffer of `cap` records (one window per pass, straight into it);
// `host`, the caller's host buffer of `cap` records, or `fn`, the caller's function -- both fed window by window through the
// workspace's stage of `stage` records per window; or nothing (`count_only`: the passes count and write no record).
struct MapSink {
  bool on = false, count_only = false, bounded = false;     // bounded: a buffer of `cap` records, too small is an error
  fa_hit_mapping *dev = nullptr, *host = nullptr;
  fa_mapping_sink fn = nullptr;
  void *user = nullptr;
  int64_t cap = 0, base = 0, stage = 0;
  int64_t *count = nullptr;
};

// One pass of the hot path over genomes [g0, g1) of a resident batch.  Everything between the first kernel and the
// final read-back is asynchronous on one stream: sizes that depend on the data (largest sketch, seed hits per
// fragment, loci, slide events) are *speculated* from earlier passes (fa_mapper::spec), checked on the device, and the
// pass is repeated with larger bounds if a check fails.  Returns the number of rows written at rows_dev[row_base ...].
//
// A pass normally covers all fragments of its genomes at once.  It is cut into *parts* (fragment ranges) when a genome
// alone holds more fragments than pass_fragments(), or when the loci / seeds / slide events of the range exceed what
// the 32-bit offsets of the workspace can address: the parts share the CGI bin table (step 2 of computeCGI is an
// atomicMax, so it simply accumulates) and the rows are formed after the last part.
//
// The pass as an object: what the stages share are its members, and the seams are its methods -- speculation (fetch_spec /
// publish_spec / scan_occupancy), the plan of the pass (plan: buffers), the launches of one part (launch_part,
// launch_rows) and the verdict on a finished part (judge_part); run() runs the parts one after another.
struct QueryPass {
  struct Range { int64_t f0, f1; bool unfused; };     // unfused: the repeat of a range that overflowed k_query_fused
  struct Run { int64_t f0, f1; Spec sp; bool with_rows; bool fused = false, forced_unfused = false, ordered = false; };
  // ---- what the caller gave ----
  fa_mapper &m;
  Workspace &w;
  const fa_genomes &g;
  const int32_t g0, g1;
  fa_cgi_row *const rows_dev;
  const int64_t cap, row_base;
  fa_cgi_row *const host_rows;
  const MapSink maps;
  // ---- constants of the pass ----
  hipStream_t st;
  const int64_t range_f0, range_f1;
  const int NQ, qcap;
  const IndexView ix;
  const int64_t npairs;
  int32_t map_chunks = 0;             // workgroups of the mapping compaction (maps.on)
  MapEmitArgs map_args;               // of the pass's last launch_maps: the later windows are written with them (stream_maps)
  int64_t nmaps = 0;                  // result: records of the pass, whatever the room
  uint64_t items_max = 0;
  size_t qs_lds = 0;
  int64_t F_total = 0;
  // ---- state of the run ----
  // the speculated bounds are shared by all workspaces: every attempt works on a copy taken under the lock and
  // publishes what it learnt (bounds only ever grow, except the LDS seed slots, which follow the latest pass)
  Spec sp;
  bool bins_cleared = false;
  bool ev_packed = false;             // the part in flight reads the packed record layout (fa_mapper::events_packed, asked once per part)
  std::deque<Range> todo;
  bool rows_valid = false;
  unsigned long long t_begin = ~0ULL, t_end = 0;
  int attempts = 0;

  QueryPass(fa_mapper &m_, Workspace &w_, const fa_genomes &g_, int32_t g0_, int32_t g1_, fa_cgi_row *rows_dev_, int64_t cap_, int64_t row_base_, fa_cgi_row *host_rows_,
            const MapSink &maps_)
      : m(m_), w(w_), g(g_), g0(g0_), g1(g1_), rows_dev(rows_dev_), cap(cap_), row_base(row_base_), host_rows(host_rows_), maps(maps_), st(w_.stream),
        range_f0(g_.genome_frag_lo[g0_]), range_f1(g_.genome_frag_lo[g1_]), NQ(g1_ - g0_), qcap(m_.qcap), ix(m_.view()), npairs((int64_t)(g1_ - g0_) * m_.G) {}

  // ================================================ speculation ================================================
  void fetch_spec() {
    std::lock_guard<std::mutex> lock(m.mtx);
    Spec &ms = m.spec;
    // (FA_SMAX_INIT: development, a smaller first guess for small fragments; FA_LOCI_CAP_MIN: the tests force the retry path
    // with a tiny value)
    if (!ms.init)
      ms = spec_first_use((int)knob::smax_init(), (int64_t)knob::loci_cap_min(), knob::events_cap_min(), pass_fragments());
    sp = ms;
    sp.fuse_off = ms.fuse_skip > 0;
    FA_REQUIRE(sp.smax < 32768, FA_ERR_UNSUPPORTED, "query sketch larger than 32767 minimizers");
    ensure_luts(m, sp.smax);
    w.lut_min_hits = m.d_min_hits.p; w.lut_pass = m.d_pass.p; w.lut_ident = m.d_ident.p;
    if (w.rules.l2_confidence != m.stats.ci) {
      // the mapper was given another interval while this call was in flight: the call keeps the one it started with
      std::vector<int32_t> own((size_t)m.stats.smax + 1);
      for (int s = 0; s <= m.stats.smax; s++) own[s] = stat_pass_threshold(s, m.stats.k, m.stats.pid, w.rules.l2_confidence);
      FA_HIP(hipStreamSynchronize(st));                        // (an earlier attempt may still read the table)
      w.own_pass.upload(own, st);
      FA_HIP(hipStreamSynchronize(st));
      w.lut_pass = w.own_pass.p;
    }
  }
  void publish_spec(const Spec &sp) {
    std::lock_guard<std::mutex> lock(m.mtx);
    spec_merge(m.spec, sp);
  }
  // workgroups per CU of the two L2 kernels at a sketch bound (their LDS grows with it), as one number; 0 = not the usual
  // instantiation (wide events, fewer than 64 loci per scan workgroup) or the runtime does not say
  int scan_occupancy(int smax) {
    if (smax + 2 >= (1 << EV_RANK16) || !m.packed_geo) return 0;
    const L2Lds lds(m.P, smax, false);
    const size_t lds_scan = lds.scan(L2_THREADS, 1), lds_ev = lds.events;
    if (lds_scan > 64 * 1024 || lds_ev > 64 * 1024) return 0;
    int n_scan = 0, n_ev = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n_scan, (const void *)k_l2_scan<uint16_t, uint8_t, 64>, L2_THREADS, lds_scan) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&n_ev, ev_packed ? (const void *)k_l2_events<uint16_t, true> : (const void *)k_l2_events<uint16_t, false>,
                                                     EV_THREADS, lds_ev) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
    }
    return n_scan > 0 && n_ev > 0 ? n_scan * 64 + n_ev : 0;
  }

  // ================================================ the plan of the pass =======================================
  void plan() {
    // event offsets are 32-bit: at most this many slide events per part (FA_EVENTS_CAP_MAX: the tests force the split)
    items_max = knob::events_cap_max();
    w.bins.ensure((size_t)NQ * std::max(m.total_bins, 1) + 2);
    w.row_count.ensure((size_t)npairs + 1); w.row_ident.ensure((size_t)npairs + 1);
    w.row_flag.ensure((size_t)npairs + 1); w.row_off.ensure((size_t)npairs + 1);
    if (maps.on) {
      // the winner table is sized and cleared with the bins; the compaction takes the bins of the pass in chunks
      const int64_t chunks = ceil_div((int64_t)NQ * m.total_bins, (int64_t)MAP_CHUNK);
      FA_REQUIRE(chunks < (1LL << 31) - 1, FA_ERR_UNSUPPORTED, "too many reference bins in one pass for the mapping output");
      map_chunks = (int32_t)chunks;
      w.winners.ensure((size_t)NQ * std::max(m.total_bins, 1) + 2);
      w.map_chunk_count.ensure((size_t)map_chunks + 1); w.map_chunk_off.ensure((size_t)map_chunks + 1);
    }
    qs_lds = (size_t)next_pow2((uint32_t)std::max(qcap, 2)) * 4;
    FA_REQUIRE(qs_lds <= 150 * 1024, FA_ERR_UNSUPPORTED, "fragment_length too large for the LDS fragment sort");

    // ---- the parts of the pass run one after another on the workspace's stream.  They share the CGI bin table (atomicMax);
    // the rows are formed behind the last part.  Every part keeps its own speculation verdict: a void part is queued again
    // (and the rows, if they were formed already, are formed again after it).
    F_total = range_f1 - range_f0;
    w.pass_F = F_total;
    // the CGI bin table is cleared once per pass, by the k_clear of the first part launched (a void first part cleared it
    // all the same)
    bins_cleared = npairs == 0;
  }

  // ================================================ launches ===================================================
  // forms the rows; returns true if the kernel also hands the pass over to the host (small passes: its last workgroup does)
  bool launch_rows(const PublishArgs &pub) {
    uint32_t *const d_counters = w.status.p->counters;
    int32_t *const d_total_rows = &w.status.p->total_rows;
    RowsArgs ra;
    ra.bins = w.bins.p; ra.genome_bin = m.genome_bin.p; ra.total_bins = m.total_bins; ra.G = m.G; ra.NQ = NQ;
    ra.row_count = w.row_count.p; ra.row_ident = w.row_ident.p;
    // small passes: the last workgroup of k_cgi_rows also forms the rows and hands the pass over -- five launches less.  Every
    // workgroup pays for it with a device-scope fence, which writes its XCD's L2 back: ~1 us each, one after another per XCD.
    // Break-even at 400-800 pairs (profiles/r05_emit_threshold.txt); at the 12-14 000 pairs of a 24-genome chunk against 500
    // references the fences were 0.44 of the 0.52 ms of the kernel.  (FA_ROWS_EMIT_MAX: the measurement's knob, <= 16384)
    ra.emit = npairs <= (int64_t)knob::rows_emit_max();
    ra.pub = pub;
    if (!ra.emit) ra.pub.seq = 0;
    ra.done = &d_counters[CNT_ROWS_DONE]; ra.query_total_frag = g.d_total_frag + g0; ra.query_id_base = g0;
    ra.rows = rows_dev + row_base; ra.cap = cap - row_base; ra.total_rows = d_total_rows;
    hipLaunchKernelGGL(k_cgi_rows, dim3(ceil_div(npairs, 4)), dim3(256), 0, st, ra);
    if (ra.emit) {
    } else {
      hipLaunchKernelGGL(k_flag_nonzero, dim3(ceil_div(npairs, 256)), dim3(256), 0, st, w.row_count.p, npairs, w.row_flag.p);
      FA_HIP(hipMemsetAsync(w.row_flag.p + npairs, 0, sizeof(int32_t), st));
      exclusive_sum_i32(w.sk.cub_temp, w.row_flag.p, w.row_off.p, (int)npairs + 1, st);
      FA_HIP(hipMemcpyAsync(d_total_rows, w.row_off.p + npairs, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(k_emit_rows, dim3(ceil_div(npairs, 256)), dim3(256), 0, st, w.row_count.p, w.row_ident.p, w.row_off.p, m.G,
                         npairs, g.d_total_frag + g0, g0, rows_dev + row_base, cap - row_base);
    }
    return ra.emit != 0;
  }
  // the mappings of the whole pass, behind its last part and in front of launch_rows (whose last workgroup may hand the
  // pass over): count per chunk, scan, and the first window of the records -- all of them for a device destination (what
  // fits its room), the first stage's worth otherwise; the total goes into the status block and travels with the hand-over,
  // and the host runs the windows behind the first once it knows it (stream_maps).  Rows that are formed again bring the
  // count, the scan and the first window again.
  void launch_maps() {
    MapEmitArgs &ea = map_args;
    ea.bins = w.bins.p; ea.winners = w.winners.p; ea.contig_genome = m.contig_genome.p;
    ea.n_bins = (int64_t)NQ * m.total_bins; ea.total_bins = std::max(m.total_bins, 1); ea.query_id_base = g0; ea.n_chunks = map_chunks;
    ea.chunk_count = w.map_chunk_count.p; ea.chunk_off = w.map_chunk_off.p;
    ea.maps = nullptr; ea.tie = TieKey::of(w.rules.cgi_ties);
    if (map_chunks) hipLaunchKernelGGL(k_map_count, dim3(map_chunks), dim3(256), 0, st, ea);
    hipLaunchKernelGGL(k_chunk_scan, dim3(1), dim3(1024), 0, st, ea.chunk_count, ea.chunk_off, ea.n_chunks, &w.status.p->total_maps);
    if (!map_chunks || maps.count_only) return;
    int64_t hi = maps.stage;
    ea.maps = w.map_stage.dev[0];
    if (maps.dev) { ea.maps = maps.dev + maps.base; hi = std::max<int64_t>(0, maps.cap - maps.base); }
    hipLaunchKernelGGL(k_map_write, dim3(map_chunks), dim3(256), 0, st, ea, (int64_t)0, hi);
  }
  // The records of the finished pass on their way to the host, window by window through the workspace's stage: window 0 lies
  // in HBM stage 0 already (launch_maps); the write of window w + 1 and its copy run while the host consumes window w.  The
  // stream is idle when this returns, so the next pass may reuse the bin and winner tables, and the next call the stage.
  void stream_maps(MapSink &sink) {
    MapStage &sg = w.map_stage;
    const int64_t total = nmaps, n_win = map_windows(total, sink.stage);
    auto issue = [&](int64_t wi) {
      const MapWindow win = map_window(total, sink.stage, wi);
      const int s = (int)(wi & 1);
      if (wi > 0) {
        MapEmitArgs ea = map_args;
        ea.maps = sg.dev[s];
        hipLaunchKernelGGL(k_map_write, dim3(map_chunks), dim3(256), 0, st, ea, win.lo, win.hi);
      }
      FA_HIP(hipMemcpyAsync(sg.pin[s], sg.dev[s], (size_t)(win.hi - win.lo) * sizeof(fa_hit_mapping), hipMemcpyDeviceToHost, st));
      FA_HIP(hipEventRecord(sg.ev[s], st));
    };
    if (n_win) issue(0);
    for (int64_t wi = 0; wi < n_win; wi++) {
      if (wi + 1 < n_win) issue(wi + 1);
      const MapWindow win = map_window(total, sink.stage, wi);
      FA_HIP(hipEventSynchronize(sg.ev[wi & 1]));
      if (sink.host) {
        memcpy(sink.host + sink.base + win.lo, sg.pin[wi & 1], (size_t)(win.hi - win.lo) * sizeof(fa_hit_mapping));
        continue;
      }
      const int rc = sink.fn(sink.user, sg.pin[wi & 1], win.hi - win.lo);
      if (rc != 0) {
        (void)hipStreamSynchronize(st);                          // (a window may be in flight: the stage is quiet before the call ends)
        throw Error(FA_ERR_INVALID, "the mapping sink ended the call (it returned " + std::to_string(rc) + ")");
      }
    }
  }
  // what the stage launches of one part share (sized by size_part)
  struct Part {
    const Spec &sp;
    const int64_t f0, f1, F;
    const int t0, ntiles;
    const int smax;
    const int64_t l_cap;
    L1Plan l1;                                                // the launches of k_l1 (plan_l1)
    bool scan_sorted = false;                                 // k_l2_scan takes its loci sorted by stream length (k_l2_order)
    bool wide = false;                                        // 32-bit slide events (wide_events)
    LociRegions loci{nullptr, 1, 0};          // regions of the locus numbering of this part
    const int32_t *frag_order = nullptr;      // workgroup order of the part (prepare_order), null = identity
    uint32_t order_len = 0;
    Part(QueryPass &q, Run &r)
        : sp(r.sp), f0(r.f0), f1(r.f1), F(r.f1 - r.f0), t0(q.g.frag_tile_lo[r.f0]),
          ntiles(q.g.frag_tile_lo[r.f1] - q.g.frag_tile_lo[r.f0]), smax(r.sp.smax),
          // (every region of the locus numbering holds at least one locus: a capacity below the number of regions -- only the
          //  FA_LOCI_CAP_MIN hook of the tests gets there -- would number loci beyond the arrays sized and cleared for l_cap)
          l_cap(std::max<int64_t>(r.sp.l_cap, (int64_t)std::min<uint32_t>(LOCI_REGIONS, ev_regions_for(r.f1 - r.f0)))) {}
  };

  // one part: its buffers, then the stages in order, then the hand-over -- all asynchronous on the workspace's stream
  void launch_part(Run &r) {
    Part p(*this, r);
    const Spec &sp = p.sp;
    const int64_t f0 = p.f0, F = p.F;
    w.last_F = 0; w.last_loci = 0;                                  // (filled in when the part is accepted)
    ev_packed = m.events_packed();
    const int ntiles = p.ntiles;
    // buffers whose size depends only on the geometry of the part
    w.sk.stage_hash.ensure((size_t)std::max(ntiles, 1) * TILE);
    w.sk.stage_wpos.ensure((size_t)std::max(ntiles, 1) * TILE);
    w.sk.tile_count.ensure((size_t)ntiles + 1);
    w.q_hash.ensure((size_t)F * qcap); w.q_off.ensure((size_t)F * qcap); w.q_cnt.ensure((size_t)F * qcap);
    w.q_size.ensure((size_t)F); w.n_seeds.ensure((size_t)F); w.ovf_off.ensure((size_t)F);
    w.f_loci_lo.ensure((size_t)F); w.f_loci_n.ensure((size_t)F);
    w.status.ensure(1);
    if (!w.h_status) {
      FA_HIP(hipHostMalloc((void **)&w.h_status, sizeof(PassStatus), hipHostMallocMapped | hipHostMallocCoherent));
      memset(w.h_status, 0, sizeof(PassStatus));
    }
    // ---- buffers and tables sized by the speculated bounds ----
    const int smax = p.smax;
    const int64_t l_cap = p.l_cap;
    {
      const L1Knobs knobs{(int)knob::l1_prefilter(), (float)knob::l1_thin_small(), (float)knob::l1_thin_mid()};
      p.l1 = plan_l1(sp, m.N, knobs);
      if (knob::debug_l1()) fprintf(stderr, "k_l1 classes: need=%u tiny=%.3f small=%.3f mid=%.3f prefilter=%d -> %d launch(es)\n", p.l1.need, sp.l1_tiny_share, sp.l1_small_share, sp.l1_mid_share, (int)p.l1.prefilter, p.l1.n);
    }
    w.l_frag.ensure((size_t)l_cap); w.l_seq.ensure((size_t)l_cap); w.l_start.ensure((size_t)l_cap); w.l_end.ensure((size_t)l_cap + 4);
    w.l_rfirst.ensure((size_t)l_cap); w.l_rlast.ensure((size_t)l_cap + 4); w.l_rpart.ensure((size_t)l_cap);
    w.l_group.ensure((size_t)l_cap); w.l_shared.ensure((size_t)l_cap); w.l_pos.ensure((size_t)l_cap);
    w.group_best.ensure((size_t)l_cap + 2);
    w.l_beg.ensure((size_t)l_cap); w.l_end0.ensure((size_t)l_cap); w.l_last.ensure((size_t)l_cap); w.l_ndrop.ensure((size_t)l_cap);
    w.l_nev.ensure((size_t)l_cap); w.l_ioff.ensure((size_t)l_cap); w.l_redo.ensure((size_t)l_cap + 4);
    p.scan_sorted = scan_sorted(sp, (int)knob::l2_scan_order());
    w.scan_hist.ensure((size_t)2 * LOCI_REGIONS * SCAN_CLASSES);
    if (p.scan_sorted) w.scan_order.ensure((size_t)l_cap + 64);
    w.ovf_buf.ensure((size_t)sp.scratch_words + 4);
    // the locus numbering: one region per sixteen fragments (64 at most), each the largest power of two that fits its share
    p.loci.count = w.status.p->loci_region;
    p.loci.n = std::min<uint32_t>(LOCI_REGIONS, ev_regions_for(F));
    p.loci.shift = (uint32_t)floor_log2((int)std::max<int64_t>(1, l_cap / p.loci.n));
    w.loci_n = p.loci.n; w.loci_shift = p.loci.shift;
    p.wide = wide_events(smax);
    w.items.ensure(((size_t)sp.items_cap + 8) * (p.wide ? 4 : 2));
    w.forms = Forms();
    w.forms.n_l1 = p.l1.n;
    for (int c = 0; c < p.l1.n; c++) w.forms.l1_threads[c] = p.l1.c[c].nt;
    w.forms.prefilter = p.l1.prefilter; w.forms.scan_sorted = p.scan_sorted; w.forms.wide = p.wide; w.forms.redo = sp.redo;
    w.forms.smax = smax; w.forms.seed_slots = p.l1.seed_slots();

    launch_sketch_stage(r, p);
    prepare_order(p);
    launch_l1_stage(p);
    launch_l2_stage(r, p);
    launch_cgi_stage_and_hand_over(r, p);
  }

  // The workgroup order of k_l2_events (frag_order_gate, build_frag_order), built on the host, cached per (batch, fragment
  // range) and uploaded behind K1.
  void prepare_order(Part &p) {
    // (FA_FRAG_ORDER_ONE: the A/B of the one-genome order)
    if (!frag_order_gate(knob::frag_order() != 0, knob::frag_order_one() != 0, NQ, p.F)) return;
    if (w.order_batch != g.serial || w.order_f0 != p.f0 || w.order_f1 != p.f1) {
      std::vector<int32_t> ord;
      w.order_len = build_frag_order(g.genome_frag_lo.data(), g0, p.f0, p.f1, ord);       // 0: the lists cannot be balanced, identity order
      if (w.order_len) {
        w.pin_order.ensure(ord.size() * sizeof(int32_t));
        memcpy(w.pin_order.p, ord.data(), ord.size() * sizeof(int32_t));
        w.frag_order.ensure(ord.size());
        FA_HIP(hipMemcpyAsync(w.frag_order.p, w.pin_order.p, ord.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
      }
      w.order_batch = g.serial; w.order_f0 = p.f0; w.order_f1 = p.f1;
    }
    if (w.order_len) { p.frag_order = w.frag_order.p; p.order_len = w.order_len; }
  }

  // K1 (its extra workgroups zero the tables of the part) + per-fragment sort / unique / index lookup
  void launch_sketch_stage(Run &r, Part &p) {
    const Spec &sp = p.sp;
    const int64_t f0 = p.f0, F = p.F;
    const int64_t l_cap = p.l_cap;
    const int t0 = p.t0, ntiles = p.ntiles;
    {
      ClearList cl;
      cl.add(w.status.p, offsetof(PassStatus, stamp));
      cl.a.stamp = &w.status.p->stamp[0];
      cl.add(w.l_end.p, (size_t)l_cap * sizeof(int32_t)); cl.add(w.l_rlast.p, (size_t)l_cap * sizeof(int32_t));
      cl.add(w.group_best.p, (size_t)l_cap * sizeof(unsigned long long));
      if (p.scan_sorted) cl.add(w.scan_hist.p, (size_t)2 * LOCI_REGIONS * SCAN_CLASSES * sizeof(uint32_t));
      if (!bins_cleared) {
        cl.add(w.bins.p, (size_t)NQ * std::max(m.total_bins, 1) * sizeof(unsigned long long));
        if (maps.on) cl.add(w.winners.p, (size_t)NQ * std::max(m.total_bins, 1) * sizeof(MapWinner));
        bins_cleared = true;
      }
      QuerySketchArgs a;
      a.frag_tile_lo = g.d_frag_tile_lo + f0;
      a.tile_count = w.sk.tile_count.p; a.stage_hash = w.sk.stage_hash.p; a.stage_wpos = w.sk.stage_wpos.p;
      a.tile_base = t0;                              // frag_tile_lo holds batch-wide tile numbers
      a.q_hash = w.q_hash.p; a.q_size = w.q_size.p; a.qcap = qcap;
      a.ix = ix; a.q_off = w.q_off.p; a.q_cnt = w.q_cnt.p; a.n_seeds = w.n_seeds.p;
      a.sort_cap = (int32_t)(qs_lds / 4);
      a.rec_cap = (int)std::max(0.0, std::min((double)QF_CAP, knob::qf_cap()));
      a.exc_tiles = 0;                                 // (set by launch_sketch_tiles for the fused kernel)
      // ---- K1 (its extra workgroups zero the ranges above beside the hashing) + per-fragment sort / unique / index lookup:
      //      one launch where the pass qualifies (k_query_fused), else k_sketch_fast / k_sketch_tiles, then k_query_sketch ----
      const bool fused = launch_sketch_tiles(m.P, g.store, g.tiles + t0, ntiles, w.sk.stage_hash.p, w.sk.stage_wpos.p, w.sk.tile_count.p, st, &cl.a,
                                             (sp.fuse_off || r.forced_unfused) ? nullptr : &a, F);
      r.fused = fused;
      if (!fused) launch_lds(k_query_sketch, dim3((unsigned)F), dim3(MAP_THREADS), qs_lds, st, a);
    }
    debug_sync(st, "sketch");
  }

  // seed totals, then the candidate regions
  void launch_l1_stage(Part &p) {
    const Spec &sp = p.sp;
    const int64_t F = p.F;
    const int smax = p.smax;
    const int64_t l_cap = p.l_cap;
    int32_t *const d_stats = w.status.p->stats;
    uint64_t *const d_totals = w.status.p->totals;
    uint32_t *const d_counters = w.status.p->counters;
    unsigned long long *const d_pinfo = w.status.p->pinfo;
    const uint32_t seed_slots = p.l1.seed_slots();
    // ---- seed totals and speculation checks (the lookup itself is the tail of k_query_sketch).  A kernel of its own
    //      only where k_l1 / k_l1_big need the scratch offsets it produces; else workgroup F of k_l1's launch ----
    const bool fold_totals = sp.scratch_words == 0;
    if (!fold_totals)
      hipLaunchKernelGGL(k_seed_totals, dim3(1), dim3(1024), 0, st, w.n_seeds.p, F, seed_slots, d_totals, w.ovf_off.p,
                         d_stats, smax, sp.scratch_words, d_pinfo, &w.status.p->stamp[1], w.q_size.p);
    debug_sync(st, "lookup");
    // ---- L1 ----
    {
      L1Args a;
      a.fold_totals = fold_totals ? 1 : 0; a.spec_smax = smax; a.F = F; a.totals = d_totals; a.stats = d_stats;
      a.spec_scratch_words = sp.scratch_words; a.stamp = &w.status.p->stamp[1];
      a.ix = ix; a.q_size = w.q_size.p; a.q_off = w.q_off.p; a.q_cnt = w.q_cnt.p; a.n_seeds = w.n_seeds.p;
      a.ovf_off = w.ovf_off.p; a.ovf_buf = w.ovf_buf.p; a.min_hits_lut = w.lut_min_hits;
      a.l_frag = w.l_frag.p; a.l_seq = w.l_seq.p; a.l_start = w.l_start.p; a.l_end = w.l_end.p; a.l_group = w.l_group.p;
      a.l_rfirst = w.l_rfirst.p; a.l_rlast = w.l_rlast.p; a.l_rpart = w.l_rpart.p;
      a.counters = d_counters; a.loci = p.loci; a.qcap = qcap; a.frag_len = m.P.fragment_length; a.l_cap = (int32_t)l_cap;
      a.lds_seed_cap = seed_slots; a.totals_seed_cap = seed_slots; a.n_lo = 0; a.n_hi = 0xFFFFFFFFu; a.pinfo = d_pinfo; a.lut_smax = smax; a.scratch_words = sp.scratch_words;
      a.f_loci_lo = w.f_loci_lo.p; a.f_loci_n = w.f_loci_n.p;
      const bool l1_block_sort_on = knob::l1_block_sort() != 0, l1_stats = knob::l1_stats() != 0;
      const bool l1_near_on = l1_near(m.N, (int)knob::l1_near());
      const bool l1_pf_on = p.l1.prefilter;             // (decided with the size classes, when the part was planned)
      a.block_sort = (l1_block_sort_on ? 1 : 0) | (l1_stats ? 2 : 0) | (l1_near_on ? 4 : 0) | (l1_pf_on ? 8 : 0);
      const uint32_t l1_grid = (uint32_t)F;             // (the offset-major order of k_l2_events applied here measured nothing: 75.9 / 75.5 ms on config 3)
      a.dbg = w.status.p->dbg;
      // fragments with more hits than LDS holds (seen before on this mapper: scratch is reserved for them) are cut
      // into LDS-sized chunks at contig boundaries by k_l1_big first; what it cannot cut stays with k_l1's HBM path
      const bool l1_big = knob::l1_big() != 0;
      a.big_state = nullptr; a.big_enabled = 0; a.big_cap = 0;
      const int64_t big_room = (int64_t)160 * 1024 - 2048 - ((int64_t)smax + 2) * 16 - (int64_t)L1_BIG_THREADS * 8;   // LDS left for a chunk's seeds
      if (l1_big && sp.scratch_words > 0 && big_room >= 4 * 2048) {
        w.big_state.ensure((size_t)F);
        a.big_cap = (uint32_t)std::min<int64_t>((int64_t)L1_BIG_E * L1_BIG_THREADS, big_room / 4 / 256 * 256);
        a.big_state = w.big_state.p; a.big_enabled = 1;
        launch_lds(k_l1_big, dim3((unsigned)F), dim3(L1_BIG_THREADS), l1_big_lds_bytes(a.big_cap, smax), st, a);
      }
      // one launch per size class (L1Class); the seed totals ride in the first one
      auto go = [&](auto nt_tag, const L1Class &c, bool fold) {
        constexpr int NTT = decltype(nt_tag)::value;
        const size_t lds = l1_lds_bytes(c.slots, smax, NTT);
        FA_REQUIRE(lds + 1024 <= 160 * 1024, FA_ERR_UNSUPPORTED, "query sketch too large for the LDS tables of the L1 kernel");
        if (knob::debug_l1()) fprintf(stderr, "k_l1<%d>: F=%lld hits %u..%u seed_slots=%u smax=%d lds=%zu\n", NTT, (long long)F, c.n_lo, c.n_hi, c.slots, smax, lds);
        L1Args b = a;
        b.lds_seed_cap = c.slots; b.n_lo = c.n_lo; b.n_hi = c.n_hi; b.fold_totals = fold ? 1 : 0;
        // (plan_l1 gives a 256-thread class L1_SMALL_HITS = 16 x 256 slots at most: it has no 32-hits-per-thread form)
        constexpr uint32_t E_MAX = NTT == 256 ? 16u : (uint32_t)L1_INPLACE_MAX;
        FA_REQUIRE(c.slots <= E_MAX * (uint32_t)NTT, FA_ERR_INTERNAL, "more seed slots than a workgroup of the L1 kernel merges");
        const auto kernel = c.slots <= 16u * (uint32_t)NTT ? k_l1<NTT, 16> : k_l1<NTT, (int)E_MAX>;
        launch_lds(kernel, dim3(l1_grid + (fold ? 1u : 0u)), dim3(NTT), lds, st, b);
      };
      for (int c = 0; c < p.l1.n; c++) {
        const bool fold = fold_totals && c == 0;
        if (p.l1.c[c].nt >= 512) go(std::integral_constant<int, 512>(), p.l1.c[c], fold);
        else go(std::integral_constant<int, 256>(), p.l1.c[c], fold);
      }
    }
    debug_sync(st, "l1");
  }

  // event streams, then the sequential slide
  void launch_l2_stage(Run &r, Part &p) {
    const Spec &sp = p.sp;
    const int64_t F = p.F;
    const int smax = p.smax;
    const int64_t l_cap = p.l_cap;
    uint64_t *const d_totals = w.status.p->totals;
    uint32_t *const d_counters = w.status.p->counters;
    unsigned long long *const d_pinfo = w.status.p->pinfo;
    const bool wide = p.wide;
    // ---- L2: event streams, then the sequential slide (uint8 state, uint16 redo) ----
    {
      if (m.stage_events) FA_HIP(hipEventRecord(w.ev[2], st));
      L2Args a;
      a.stamp = &w.status.p->stamp[2];
      a.ix = ix; a.q_hash = w.q_hash.p; a.q_size = w.q_size.p;
      a.l_frag = w.l_frag.p; a.l_seq = w.l_seq.p; a.l_start = w.l_start.p; a.l_end = w.l_end.p; a.l_group = w.l_group.p;
      a.l_rfirst = w.l_rfirst.p; a.l_rlast = w.l_rlast.p; a.l_rpart = w.l_rpart.p; a.frag_len = m.P.fragment_length;
      a.l_beg = w.l_beg.p; a.l_end0 = w.l_end0.p; a.l_last = w.l_last.p; a.l_nev = w.l_nev.p; a.l_ioff = w.l_ioff.p; a.l_ndrop = w.l_ndrop.p;
      a.items = w.items.p; a.items_cap = sp.items_cap; a.pinfo = d_pinfo; a.l_cap = (int32_t)l_cap;
      a.l_shared = w.l_shared.p; a.l_pos = w.l_pos.p; a.pass_lut = w.lut_pass; a.group_best = w.group_best.p;
      a.counters = d_counters; a.loci = p.loci; a.qcap = qcap; a.cmw = m.cmw;
      a.cnt_slots = smax + 1;
      a.rec_total = (unsigned long long *)&d_totals[TOT_RECORDS];
      a.ev_region = w.status.p->ev_region; a.rec_region = w.status.p->rec_region;
      a.n_regions = ev_regions_for(F);
      a.region_cap = (sp.items_cap / a.n_regions) & ~7ULL;
      a.l_redo = w.l_redo.p;
      a.redo_count = &d_counters[CNT_WIDE];
      const L2Lds lds(m.P, smax, wide);
      a.scan_class_div = p.scan_sorted ? lds.scan_class_div : 0;
      a.scan_hist = w.scan_hist.p; a.scan_cursor = w.scan_hist.p + LOCI_REGIONS * SCAN_CLASSES;
      a.scan_order = p.scan_sorted ? w.scan_order.p : nullptr;
      a.slide_end = w.rules.slide_end; a.tie = TieKey::of(w.rules.cgi_ties);
      a.f_loci_lo = w.f_loci_lo.p; a.f_loci_n = w.f_loci_n.p;
      // several genomes in the pass: the workgroups of k_l2_events in offset-major order (prepare_order)
      a.frag_order = p.frag_order;
      const uint32_t ev_grid = p.frag_order ? p.order_len : (uint32_t)F;
      if (p.frag_order) r.ordered = true;
      a.ev_stage = lds.ev_stage;
      const size_t ev_lds = lds.events;
      FA_REQUIRE(ev_lds <= 150 * 1024, FA_ERR_UNSUPPORTED, "query sketch too large for the LDS-staged event kernel");
      // fast pass: one state byte per rank; redo pass: two bytes per rank, only for loci whose counts overflowed
      auto pick_lanes = [&](int bytes) {
        int ln = L2_THREADS;
        while (ln > 1 && lds.scan(ln, bytes) > 144 * 1024) ln >>= 1;   // large sketches (tiny windows): fewer loci per workgroup
        FA_REQUIRE(lds.scan(ln, bytes) <= 160 * 1024, FA_ERR_UNSUPPORTED, "query sketch too large for the LDS-resident L2 state");
        return ln;
      };
      const int lanes8 = pick_lanes(1), lanes16 = pick_lanes(2);
      const size_t lds8 = lds.scan(lanes8, 1), lds16 = lds.scan(lanes16, 2);
      // (workgroup b of a scan takes chunk b / n of region b mod n: every region needs its chunks, however few loci it can hold)
      auto scan_grid = [&](int lanes) { return (unsigned)(p.loci.n * (uint32_t)ceil_div((int64_t)1 << p.loci.shift, lanes)); };
      auto launch = [&](auto ev_kernel, auto scan8, auto scan8_rt, auto scan16, auto scan16_rt) {
        launch_lds(ev_kernel, dim3(ev_grid), dim3(EV_THREADS), ev_lds, st, a);
        debug_sync(st, "l2 events");
        if (p.scan_sorted)
          hipLaunchKernelGGL(k_l2_order, dim3((unsigned)(p.loci.n * (uint32_t)ceil_div((int64_t)1 << p.loci.shift, 256))), dim3(256), 0, st, a);
        // the number of loci is only known on the device: launch for the capacity, surplus workgroups exit at once
        a.lanes = lanes8;
        launch_lds(lanes8 == L2_THREADS ? scan8 : scan8_rt, dim3(scan_grid(lanes8)), dim3(L2_THREADS), lds8, st, a);
        // the wide-state pass is only launched once some locus has needed it (a part that finds out too late is repeated)
        if (!sp.redo) return;
        a.lanes = lanes16;
        launch_lds(lanes16 == L2_THREADS ? scan16 : scan16_rt, dim3(scan_grid(lanes16)), dim3(L2_THREADS), lds16, st, a);
      };
      const bool pk = ev_packed;
      if (wide) launch(pk ? k_l2_events<uint32_t, true> : k_l2_events<uint32_t, false>, k_l2_scan<uint32_t, uint8_t, 64>, k_l2_scan<uint32_t, uint8_t, 0>, k_l2_scan<uint32_t, uint16_t, 64>, k_l2_scan<uint32_t, uint16_t, 0>);
      else launch(pk ? k_l2_events<uint16_t, true> : k_l2_events<uint16_t, false>, k_l2_scan<uint16_t, uint8_t, 64>, k_l2_scan<uint16_t, uint8_t, 0>, k_l2_scan<uint16_t, uint16_t, 64>, k_l2_scan<uint16_t, uint16_t, 0>);
    }
    debug_sync(st, "l2 scan");
    if (m.stage_events) FA_HIP(hipEventRecord(w.ev[3], st));
  }

  // core-genome identity and the one hand-over of the part
  void launch_cgi_stage_and_hand_over(Run &r, Part &p) {
    const Spec &sp = p.sp;
    const int64_t f0 = p.f0;
    const int64_t l_cap = p.l_cap;
    uint32_t *const d_counters = w.status.p->counters;
    // ---- core-genome identity ----
    if (npairs > 0) {
      CgiArgs a;
      a.stamp = &w.status.p->stamp[3];
      a.ix = ix; a.group_best = w.group_best.p; a.counters = d_counters; a.l_frag = w.l_frag.p; a.l_seq = w.l_seq.p;
      a.l_pos = w.l_pos.p; a.q_size = w.q_size.p; a.ident_lut = w.lut_ident;
      a.frag_query = g.d_frag_query + f0; a.frag_qseq = g.d_frag_qseq + f0; a.bins = w.bins.p;
      a.bin_len = m.P.fragment_length - 20;
      a.query_base = g0;                             // frag_query holds batch-wide genome numbers
      a.wide_launched = sp.redo ? 1 : 0;
      a.tie = TieKey::of(w.rules.cgi_ties);
      a.group_bound = p.loci.n << p.loci.shift;
      hipLaunchKernelGGL(k_cgi_bins, dim3(ceil_div(l_cap, 256)), dim3(256), 0, st, a);
      if (maps.on) hipLaunchKernelGGL(k_cgi_winners, dim3(ceil_div(l_cap, 256)), dim3(256), 0, st, a, w.winners.p);
    }
    // ---- the one hand-over of the part: results, statistics and the speculation verdict (publish_pass) ----
    if (r.with_rows) rows_valid = true;
    hand_over(r.with_rows);
  }
  // hands the pass over to the host (publish_args): with `rows` the rows are formed first (launch_rows, whose last workgroup
  // hands over for small passes); otherwise k_publish_status does
  void hand_over(bool rows) {
    PassStatus *h_dev = nullptr;
    FA_HIP(hipHostGetDevicePointer((void **)&h_dev, w.h_status, 0));
    const PublishArgs pub = publish_args(w.status.p, h_dev, ++w.seq, rows_dev + row_base, rows && host_rows ? host_rows + row_base : nullptr, cap - row_base);
    if (rows && maps.on) launch_maps();
    const bool published = rows && launch_rows(pub);
    FA_HIP(hipGetLastError());
    debug_sync(st, "cgi");
    if (!published) hipLaunchKernelGGL(k_publish_status, dim3(1), dim3(256), 0, st, pub);
  }

  // ================================================ the verdict on a part ======================================
  // waits for a part and reads its verdict: true = accepted, false = void (its range has to run again)
  bool judge_part(Run &r) {
    Spec &sp = r.sp;
    const int64_t F = r.f1 - r.f0;
    wait_published(w.h_status, w.seq, w.stream);
    const PassStatus &h = *w.h_status;
    const Verdict v = judge(sp, h, w.forms, F, w.loci_n, w.loci_shift, items_max, [&](int s) { return scan_occupancy(s); });
    if (v.miss) w.last_ms[MS_REPEATS] += 1.0f;   // repeated attempts of this call (speculation misses)
    if (v.fuse_overflow) {
      r.forced_unfused = true;                           // this range again, through the two kernels
      std::lock_guard<std::mutex> lock(m.mtx);
      fuse_overflowed(m.spec);
    }
    FA_REQUIRE(v.kind != Verdict::FAILED, FA_ERR_UNSUPPORTED, std::string("a single query fragment produces too many ") + v.what);
    publish_spec(sp);
    if (v.kind != Verdict::ACCEPTED) return false;      // void part: run it again
    // ---- accepted ----
    {
      std::lock_guard<std::mutex> lock(m.mtx);
      fuse_accepted(m.spec, r.fused, sp.fuse_off && !r.forced_unfused);
    }
    w.last_ms[r.fused ? MS_FUSED : MS_UNFUSED] += 1.0f;
    if (r.ordered) w.last_ms[MS_ORDERED] += 1.0f;
    w.last_forms = w.forms;
    w.last_forms.fused = r.fused; w.last_forms.ordered = r.ordered;
    if (m.stage_events) {
      float ev_ms = 0;
      FA_HIP(hipEventSynchronize(w.ev[3]));
      FA_HIP(hipEventElapsedTime(&ev_ms, w.ev[2], w.ev[3]));
      w.last_ms[MS_L2_EVENTS] += ev_ms;
    }
    const unsigned long long *stamp = h.stamp;                         // 100 MHz ticks
    for (int i = 0; i < 4; i++) w.last_ms[MS_STAGE + i] += (float)((double)(stamp[i + 1] - stamp[i]) * 1e-5);
    t_begin = std::min(t_begin, stamp[0]); t_end = std::max(t_end, stamp[4]);
    w.last_F = F;
    w.last_loci = (uint32_t)v.loci;
    for (uint32_t i = 0; i < LOCI_REGIONS; i++)
      w.last_region_count[i] = i < w.loci_n ? (uint32_t)std::min<uint64_t>(h.loci_region[i], 1ULL << w.loci_shift) : 0u;
    w.last_items = v.events;
    const uint32_t *c = h.counters;
    w.last_ms[MS_RECORDS] += (float)v.records;   // reference records inside the locus ranges of this call (roofline line)
    w.last_ms[MS_LOCI] += (float)v.loci;
    w.last_ms[MS_EVENTS] += (float)v.events;     // slide events
    w.last_ms[MS_WIDE] += (float)c[CNT_WIDE];   // loci that needed the wide L2 state
    w.last_ms[MS_L1_SORTED] += (float)c[CNT_L1_SORTED]; w.last_ms[MS_L1_MERGED] += (float)c[CNT_L1_MERGED];   // FA_L1_STATS=1: fragments block-sorted / merged by k_l1
    w.last_ms[MS_L1_OFF_FAST] += (float)(c[CNT_MERGED] + c[CNT_OFF_FAST]);   // fragments that left k_l1's fast form (exact): merged in LDS, HBM road, k_l1_big
    if (c[CNT_L1_SORTED] + c[CNT_L1_MERGED] > 0) {
      const double nf = (double)(c[CNT_L1_SORTED] + c[CNT_L1_MERGED]);
      fprintf(stderr, "[fa] k_l1 phases, shader-clock ticks per fragment (thread 0):");
      for (int i = 0; i < 8; i++) fprintf(stderr, " %.0f", (double)h.dbg[i] / nf);
      fprintf(stderr, "  (%u block-sorted, %u merged; one workgroup in 64 sampled; gave up on probes / blocks / counts: %llu %llu %llu; expansion: bitmaps+places %.0f, pairs+bitmaps %.0f, bits %.0f)\n",
              c[CNT_L1_SORTED], c[CNT_L1_MERGED], h.dbg[8], h.dbg[9], h.dbg[10], (double)h.dbg[11] / nf, (double)h.dbg[12] / nf, (double)h.dbg[13] / nf);
    }
    return true;
  }


  // ================================================ the pass ===================================================
  int64_t run() {
    w.last_F = 0; w.last_loci = 0; w.last_genomes = &g;
    for (int i = 0; i < 6; i++) if (!w.ev[i]) FA_HIP(hipEventCreate(&w.ev[i]));
    if (range_f1 == range_f0) return 0;
    FA_REQUIRE(m.P.fragment_length > 20, FA_ERR_UNSUPPORTED, "fragment_length must exceed 20 (the reference bins by fragment_length - 20)");
    fetch_spec();
    plan();
    todo.push_back(Range{range_f0, range_f1, false});
    while (!todo.empty()) {
      FA_REQUIRE(attempts < 40 + 4 * (int)(F_total / std::max<int64_t>(1, std::min(F_total, sp.part_frags)) + 1), FA_ERR_INTERNAL,
                 "query pass did not converge on its buffer sizes");
      attempts++;
      fetch_spec();
      const Range range = todo.front(); todo.pop_front();
      const int64_t f1 = std::min(range.f1, range.f0 + std::max<int64_t>(1, sp.part_frags));
      if (f1 < range.f1) todo.push_front(Range{f1, range.f1, range.unfused});
      Run r{range.f0, f1, sp, todo.empty() && npairs > 0};
      r.forced_unfused = range.unfused;
      if (r.with_rows) rows_valid = false;
      launch_part(r);
      if (!judge_part(r)) {
        todo.push_front(Range{r.f0, r.f1, r.forced_unfused});
        rows_valid = false;                     // (rows formed before lack this part)
      }
    }
    int64_t nrows = 0;
    if (npairs > 0) {
      if (!rows_valid) {
        // a part was repeated after the rows had been formed: form them again, behind everything
        FA_HIP(hipMemsetAsync(&w.status.p->counters[CNT_ROWS_DONE], 0, sizeof(uint32_t), st));
        FA_HIP(hipMemsetAsync(&w.status.p->total_rows, 0, sizeof(int32_t), st));
        hand_over(true);
        wait_published(w.h_status, w.seq, st);
      }
      nrows = w.h_status->total_rows;
      if (maps.on) nmaps = w.h_status->total_maps;
    }
    if (t_end > t_begin) w.last_ms[MS_TOTAL] += (float)((double)(t_end - t_begin) * 1e-5);   // device wall time of the pass
    FA_REQUIRE(nrows <= cap - row_base, FA_ERR_INVALID, "row buffer too small");
    return nrows;
  }
};

// (the records of the pass are appended to `maps`, whose base moves on; the caller learns the count before a destination
// that is too small is refused)
static int64_t run_query_pass(fa_mapper &m, Workspace &w, const fa_genomes &g, int32_t g0, int32_t g1, fa_cgi_row *rows_dev, int64_t cap,
                              int64_t row_base, fa_cgi_row *host_rows, MapSink &maps) {
  QueryPass pass(m, w, g, g0, g1, rows_dev, cap, row_base, host_rows, maps);
  const int64_t nrows = pass.run();
  if (maps.on) {
    *maps.count = maps.base + pass.nmaps;
    if (maps.bounded) FA_REQUIRE(pass.nmaps <= maps.cap - maps.base, FA_ERR_INVALID, "mapping buffer too small");
    if (maps.host || maps.fn) pass.stream_maps(maps);
    maps.base += pass.nmaps;
  }
  return nrows;
}

// The mappings a call asked for: the destination as the caller gave it -- a buffer of `cap` records on the device or the
// host (fa_mapper_query_mappings), or, with `stream`, the function `fn` (fa_mapper_query_mappings_stream; null: count only).
struct MapRequest {
  fa_hit_mapping *maps; int64_t cap; int64_t *n_maps; bool device;
  bool stream = false; fa_mapping_sink fn = nullptr; void *user = nullptr;
};

static int64_t run_query(fa_mapper &m, Workspace &w, const fa_genomes &g, int32_t first, int32_t count, fa_cgi_row *rows, int64_t cap, bool rows_device,
                         const MapRequest *want = nullptr) {
  require_device();
  FA_REQUIRE(first >= 0 && count >= 0 && first + count <= g.n_genomes, FA_ERR_INVALID, "genome range out of bounds");
  for (float &x : w.last_ms) x = 0;
  w.last_forms = Forms();
  { std::lock_guard<std::mutex> lock(m.mtx); w.rules = m.rules; }   // the rules in force when the call starts hold for all of it
  fa_cgi_row *dst = rows;
  if (!rows_device) { w.rows_dev.ensure((size_t)std::max<int64_t>(cap, 1)); dst = w.rows_dev.p; }
  // a call that is ONE pass and returns a modest number of rows to the host gets them written into pinned memory by the
  // pass's last kernel (k_publish_status): no device-to-host copy, no second synchronisation
  const bool one_pass = count > 0 && g.genome_frag_lo[first + count] - g.genome_frag_lo[first] <= pass_fragments();
  fa_cgi_row *host_rows = nullptr;
  if (!rows_device && one_pass && cap <= 65536) {
    w.pin_rows.ensure(std::max<size_t>((size_t)cap * sizeof(fa_cgi_row), 4096));
    FA_HIP(hipHostGetDevicePointer((void **)&host_rows, w.pin_rows.p, 0));
  }
  MapSink sink;
  if (want) {
    FA_REQUIRE(want->n_maps && (want->stream || (want->cap >= 0 && (want->maps || want->cap == 0))), FA_ERR_INVALID, "mapping buffer missing");
    sink.on = true; sink.count = want->n_maps;
    if (want->stream) { sink.fn = want->fn; sink.user = want->user; sink.count_only = !want->fn; }
    else if (want->device) { sink.bounded = true; sink.dev = want->maps; sink.cap = want->cap; sink.count_only = !want->maps; }
    else { sink.bounded = true; sink.host = want->maps; sink.cap = want->cap; sink.count_only = !want->maps; }   // (no buffer, no room: the count is all there is)
    {
      std::lock_guard<std::mutex> lock(m.mtx);
      sink.stage = m.map_stage;
      m.last_map_ws = (int)(&w - m.ws);
    }
    if (sink.host || sink.fn) w.map_stage.resize(sink.stage);
    *want->n_maps = 0;
  }
  int64_t nrows = 0;
  int32_t g0 = first;
  while (g0 < first + count) {
    int32_t g1 = g0 + 1;
    while (g1 < first + count && g.genome_frag_lo[g1 + 1] - g.genome_frag_lo[g0] <= pass_fragments()) g1++;
    // frag_query is batch-wide: the bins of a pass are indexed by (genome - g0), handled through the pointer offset below
    nrows += run_query_pass(m, w, g, g0, g1, dst, cap, nrows, host_rows, sink);
    g0 = g1;
  }
  if (!rows_device && nrows) {
    const size_t bytes = (size_t)nrows * sizeof(fa_cgi_row);
    if (!host_rows || nrows > ROWS_INLINE_MAX) {
      // through pinned memory: a device-to-pageable copy of a few KB costs more in staging than the copy itself
      // (host_rows set: the publishing workgroup leaves more than ROWS_INLINE_MAX rows to this copy)
      w.pin_rows.ensure(std::max<size_t>(bytes, 4096));
      FA_HIP(hipMemcpyAsync(w.pin_rows.p, w.rows_dev.p, bytes, hipMemcpyDeviceToHost, w.stream));
      FA_HIP(hipStreamSynchronize(w.stream));
    }
    memcpy(rows, w.pin_rows.p, bytes);
  }
  return nrows;
}

// A query call borrows one workspace of the mapper for its duration (blocks while all are busy): fa_lease.h.
struct WorkspaceLease : Lease<fa_mapper, Workspace> {
  explicit WorkspaceLease(fa_mapper &mm)
      : Lease<fa_mapper, Workspace>((bind_device(mm.device), mm), [](Workspace &w) {
          if (!w.stream && hipStreamCreate(&w.stream) != hipSuccess) {
            (void)hipGetLastError();
            w.stream = nullptr;
            throw Error(FA_ERR_NO_DEVICE, "hipStreamCreate failed");
          }
        }) {}
};

// pack + cut into fragments + tiles + upload, in place: `g` may be a batch object whose device buffers are recycled, contents
// replaced.  That and `pin` (pinned staging memory the image is built in, so that the one upload is a plain DMA) serve the
// one-query-at-a-time call; without `pin` the image is built in pageable memory.
// `packed` (fa_genomes_upload_fasta): contig c is record packed[c] of a file that read_fasta_packed has packed already -- its
// words are copied where `contigs` would be packed; `contigs` is not read then.
// `sync_pinned` (fa_genomes_reload_fasta: device buffers, pinned image and upload stream are recycled from chunk to chunk): wait
// for the upload although the image is pinned (the image is reused next).
static void fill_genomes(fa_genomes *g, const fa_params &P, hipStream_t st, const void *const *contigs, const int64_t *lengths,
                         const int32_t *contig_genome, int64_t n_contigs, int32_t n_genomes, int width,
                         float *host_ms, PinnedBuf *pin, const PackedRef *packed, bool sync_pinned) {
  require_device();
  const auto t_begin = std::chrono::steady_clock::now();
  auto lap = [&, last = t_begin](int slot) mutable {
    const auto now = std::chrono::steady_clock::now();
    if (host_ms) host_ms[slot] = std::chrono::duration<float, std::milli>(now - last).count();
    last = now;
  };
  FA_REQUIRE(width == 1 || width == 2 || width == 4, FA_ERR_INVALID, "char_width must be 1, 2 or 4");
  g->P = P;
  g->serial = ++g_batch_serial;
  // which contigs are mapped, how many whole fragments each holds, the per-genome counters and every size of the image
  BatchPlan plan = plan_batch(P, lengths, contig_genome, n_contigs, n_genomes, TILE, sizeof(Tile));
  const BatchLayout &at = plan.at;
  const int64_t F = plan.F, ntiles = plan.ntiles, tiles_per_frag = plan.tiles_per_frag;
  const int frag = P.fragment_length;
  g->n_genomes = n_genomes;
  g->F = F; g->ntiles = ntiles; g->total_bases = plan.total_bases;
  g->genome_frag_lo = std::move(plan.genome_frag_lo); g->contig_frag_lo = std::move(plan.contig_frag_lo);
  g->total_fragments = std::move(plan.total_fragments); g->total_length = std::move(plan.total_length); g->n_short = std::move(plan.n_short);
  HostStore hs;
  hs.protein = P.alphabet_size != 4;
  const size_t image_bytes = at.image_bytes, bases = plan.bases;
  unsigned char *img;
  if (pin) { pin->ensure(image_bytes); img = pin->p; }
  else { g->host_image.resize(image_bytes); img = g->host_image.data(); }
  StageTrace tr("upload_genomes");
  // the slack behind the packed words / bytes (the sketch kernel's funnel shift reads one word past the end)
  if (!hs.protein) memset(img + at.packed.at + bases / 4, 0, at.packed.bytes - bases / 4); else memset(img + at.bytes.at + bases, 0, at.bytes.bytes - bases);
  if (packed) {
    std::vector<PackedRef> use_ref;
    for (const ContigJob &cj : plan.jobs) use_ref.push_back(PackedRef{packed[cj.c].file, packed[cj.c].rec, cj.nfrag * frag});
    place_packed(hs, use_ref.data(), (int64_t)use_ref.size(), (uint32_t *)(img + at.packed.at), img + at.bytes.at);
  } else {
    std::vector<const void *> use_ptr;
    for (const ContigJob &cj : plan.jobs) use_ptr.push_back(contigs[cj.c]);
    hs.pack_many(use_ptr.data(), plan.use_len.data(), (int64_t)use_ptr.size(), width, (uint32_t *)(img + at.packed.at), img + at.bytes.at);
  }
  tr.mark("pack", st);
  lap(0);
  // fragments and tiles, written straight into the image by the host pool (1.7 M fragments and 5 M tiles for a thousand
  // genomes were one thread's loop)
  Tile *tiles = (Tile *)(img + at.tiles.at);
  int32_t *frag_query = (int32_t *)(img + at.frag_query.at), *frag_qseq = (int32_t *)(img + at.frag_qseq.at), *tf = (int32_t *)(img + at.total_frag.at);
  g->frag_tile_lo.assign((size_t)F + 1, 0);
  HostPool::get().parallel_for(plan.jobs.size(), [&](size_t j) {
    const ContigJob &cj = plan.jobs[j];
    for (int64_t i = 0; i < cj.nfrag; i++) {
      const int64_t f = cj.nf0 + i;
      g->frag_tile_lo[(size_t)f] = (int32_t)(f * tiles_per_frag);
      make_tiles_at(tiles + f * tiles_per_frag, hs, hs.seq_off[cj.si] + i * frag, frag, (int)f, P.kmer_size, P.window_size);
      frag_qseq[f] = (int32_t)(cj.q0 + i);
      frag_query[f] = cj.gi;
    }
  });
  g->frag_tile_lo[(size_t)F] = (int32_t)ntiles;
  memcpy(img + at.frag_tile_lo.at, g->frag_tile_lo.data(), ((size_t)F + 1) * 4);
  for (int i = 0; i < n_genomes; i++) tf[i] = (int32_t)g->total_fragments[i];
  tr.mark("fragments_tiles", st);
  lap(1);
  g->blob.ensure(image_bytes);
  // The one-query call (image in the workspace's pinned block, untouched until the call returns): the sketch stage reads the
  // packed words STRAIGHT from the pinned image over PCIe -- every word is read once, by the workgroup that hashes it, and the
  // kernel is bound by its hashing, so the 1.25 MB travel inside its 67 us instead of in a 28 us copy in front of it; only the
  // tile and fragment tables (read by every stage) are copied.  FA_QUERY_ZERO_COPY=0: the whole image is copied.
  const bool zero_copy = knob::query_zero_copy() != 0 && pin && !sync_pinned && !hs.protein;
  if (zero_copy) FA_HIP(hipMemcpyAsync(g->blob.p + at.tiles.at, img + at.tiles.at, image_bytes - at.tiles.at, hipMemcpyHostToDevice, st));
  else FA_HIP(hipMemcpyAsync(g->blob.p, img, image_bytes, hipMemcpyHostToDevice, st));
  const int64_t n_exc = (int64_t)hs.exc_pos.size();
  if (n_exc) { g->exc_pos.upload(hs.exc_pos, st); g->exc_val.upload(hs.exc_val, st); }
  g->store = StoreView();
  g->store.packed = hs.protein ? nullptr : (const uint32_t *)((zero_copy ? img : g->blob.p) + at.packed.at);
  g->store.bytes = hs.protein ? (const uint8_t *)(g->blob.p + at.bytes.at) : nullptr;
  g->store.exc_pos = g->exc_pos.p; g->store.exc_val = g->exc_val.p; g->store.n_exc = n_exc;
  g->tiles = (const Tile *)(g->blob.p + at.tiles.at);
  g->d_frag_tile_lo = (const int32_t *)(g->blob.p + at.frag_tile_lo.at);
  // the CGI bins of a pass are indexed by the genome number relative to the first genome of the pass; passes start at
  // genome boundaries, so the per-fragment genome numbers are batch-wide and the kernel subtracts the pass's first genome
  g->d_frag_query = (const int32_t *)(g->blob.p + at.frag_query.at);
  g->d_frag_qseq = (const int32_t *)(g->blob.p + at.frag_qseq.at);
  g->d_total_frag = (const int32_t *)(g->blob.p + at.total_frag.at);
  // the staging image must stay untouched until the copy has left it (pageable copies return after staging, pinned ones
  // are asynchronous).  An image in the caller's pinned block (the one-query call: the block belongs to the workspace and
  // is not touched again before the call returns, and the pass runs on this same stream, behind the copy) needs no
  // synchronisation; otherwise one per upload
  if (!pin || sync_pinned) {
    FA_HIP(hipStreamSynchronize(st));
    std::vector<unsigned char, NoInitAlloc<unsigned char>>().swap(g->host_image);
  }
  tr.mark("uploads", st);
  lap(2);
}

// the records of packed files as one contig list, one genome per file
struct PackedContigs {
  std::vector<PackedRef> refs;
  std::vector<int64_t> lens;
  std::vector<int32_t> genome;
  PackedContigs(const PackedFasta *files, int32_t n_paths) {
    for (int32_t i = 0; i < n_paths; i++)
      for (size_t r = 0; r < files[i].rec_len.size(); r++) { refs.push_back(PackedRef{&files[i], (int64_t)r, files[i].rec_len[r]}); lens.push_back(files[i].rec_len[r]); genome.push_back(i); }
  }
};
// one genome per FASTA file, every file read + packed by its own task of the host pool (read_fasta_packed_many), then the
// batch image assembled from the packed records and uploaded on the batch's own stream
// genomes [first, first + count) of files packed already (one genome per file) as the batch `g`
static void fill_genomes_from_packed(fa_mapper *m, fa_genomes *g, const PackedFasta *files, int32_t n_paths, bool pinned) {
  const PackedContigs all(files, n_paths);
  bind_device(m->device);
  // (its own stream: a batch may be uploaded while another thread maps the previous one, Mapper.query_fasta_stream)
  if (!g->up_stream) FA_HIP(hipStreamCreateWithFlags(&g->up_stream, hipStreamNonBlocking));
  fill_genomes(g, m->P, g->up_stream, nullptr, all.lens.data(), all.genome.data(), (int64_t)all.refs.size(), n_paths, 1, nullptr,
               pinned ? &g->pin_image : nullptr, all.refs.data(), true);
}
static void fill_genomes_from_fasta(fa_mapper *m, fa_genomes *g, const char *const *paths, int32_t n_paths, bool pinned) {
  std::vector<PackedFasta> files;
  read_fasta_packed_many(paths, (size_t)n_paths, m->P.alphabet_size != 4, files);
  fill_genomes_from_packed(m, g, files.data(), n_paths, pinned);
}

// FASTA files read and packed ONCE, to be used as references AND as queries (an all-vs-all reads every file one time)
struct fa_packed {
  bool protein = false;
  std::vector<PackedFasta> files;
  // fa_packed_append grows `files` (and moves every PackedFasta) under the exclusive lock; the calls that read them
  // (fa_packed_info, fa_sketch_add_packed, fa_genomes_reload_packed -- all run without the GIL) hold it shared for their duration
  std::shared_mutex mtx;
};
// the bookkeeping of fa_sketch_add_fasta_many over files that are packed already (s->mtx held by the caller)
static void sketch_add_packed_files(fa_sketch *s, const PackedFasta *files, int32_t n_paths, int64_t *n_records, int64_t *n_short) {
  const PackedContigs all(files, n_paths);
  std::vector<PackedRef> refs;
  RefStage add(s->book, OpenGenome::REFUSE, n_paths);
  add.genomes(s->P, all.lens.data(), all.genome.data(), (int64_t)all.refs.size(), n_paths, [&](int64_t c) { refs.push_back(all.refs[(size_t)c]); });
  add.commit(s->book, [&] { if (!refs.empty()) append_packed(s->pending, refs.data(), (int64_t)refs.size()); });
  for (int32_t i = 0; i < n_paths; i++) {
    if (n_records) n_records[i] = (int64_t)files[i].rec_len.size();
    if (n_short) n_short[i] = add.n_short[(size_t)i];
  }
}

// ------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------
// the live loci of a part, region by region (LociRegions): fn(first locus number, count)
template <class Fn>
static void for_each_locus_slice(const Workspace &x, Fn fn) {
  for (uint32_t r = 0; r < x.loci_n && r < (uint32_t)LOCI_REGIONS; r++)
    if (x.last_region_count[r]) fn((size_t)r << x.loci_shift, (size_t)x.last_region_count[r]);
}

extern "C" {

const char *fa_last_error(void) { return g_last_error.c_str(); }
int fa_version(void) { return 100; }
int fa_device_trim(uint64_t *held_bytes) {
  return guarded([&] {
    if (held_bytes) *held_bytes = (uint64_t)DevPool::get().held();
    DevPool::get().trim();
  });
}

int fa_device_count(int *count) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
  *count = n;
  return FA_OK;
}
int fa_set_device(int device) {
  return guarded([&] { require_device(); FA_HIP(hipSetDevice(device)); g_device.store(device); });
}

int fa_recommended_window_size(double p_value, int k, int alphabet_size, float identity, int fragment_length,
                               uint64_t reference_size, int *window) {
  return guarded([&] { *window = stat_recommended_window(p_value, k, alphabet_size, identity, fragment_length, reference_size); });
}
int fa_estimate_minimum_hits_relaxed(int s, int k, float identity, int *hits) {
  return guarded([&] { *hits = stat_min_hits_relaxed(s, k, identity); });
}
int fa_mapping_identity(int shared, int s, int k, float *identity, float *upper) {
  return guarded([&] { FA_REQUIRE(s > 0, FA_ERR_INVALID, "sketch_size must be positive"); stat_identity(shared, s, k, identity, upper); });
}

// host twin of the device hash (same published algorithm as fa_sketch.hip.h's Murmur)
uint32_t fa_hash(const void *kmer, int len) {
  const uint8_t *d = (const uint8_t *)kmer;
  auto rotl = [](uint64_t x, int r) { return (x << r) | (x >> (64 - r)); };
  auto fmix = [](uint64_t k) { k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33; return k; };
  const uint64_t c1 = 0x87c37b91114253d5ULL, c2 = 0x4cf5ad432745937fULL;
  uint64_t h1 = 42, h2 = 42;
  int nb = len / 16;
  for (int i = 0; i < nb; i++) {
    uint64_t k1, k2;
    memcpy(&k1, d + 16 * i, 8); memcpy(&k2, d + 16 * i + 8, 8);
    k1 *= c1; k1 = rotl(k1, 31); k1 *= c2; h1 ^= k1; h1 = rotl(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
    k2 *= c2; k2 = rotl(k2, 33); k2 *= c1; h2 ^= k2; h2 = rotl(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
  }
  const uint8_t *t = d + 16 * nb;
  int rem = len & 15;
  uint64_t k1 = 0, k2 = 0;
  for (int j = 0; j < rem; j++) { if (j < 8) k1 |= (uint64_t)t[j] << (8 * j); else k2 |= (uint64_t)t[j] << (8 * (j - 8)); }
  if (rem > 8) { k2 *= c2; k2 = rotl(k2, 33); k2 *= c1; h2 ^= k2; }
  if (rem > 0) { k1 *= c1; k1 = rotl(k1, 31); k1 *= c2; h1 ^= k1; }
  h1 ^= (uint64_t)len; h2 ^= (uint64_t)len; h1 += h2; h2 += h1; h1 = fmix(h1); h2 = fmix(h2);
  return (uint32_t)(h1 + h2);
}

int fa_sketch_new(const fa_params *params, fa_sketch **out) {
  return guarded([&] {
    validate_params(*params);
    std::unique_ptr<fa_sketch> s(new fa_sketch());
    s->P = *params;
    s->device = g_device.load();
    s->reset_data();
    *out = s.release();
  });
}
void fa_sketch_free(fa_sketch *s) {
  if (!s) return;
  if (s->stream) (void)hipStreamDestroy(s->stream);
  if (s->up_stream) (void)hipStreamDestroy(s->up_stream);
  delete s;
}
int fa_sketch_add_contig(fa_sketch *s, const void *data, int64_t length, int char_width, int *added) {
  return guarded([&] {
    FA_REQUIRE(char_width == 1 || char_width == 2 || char_width == 4, FA_ERR_INVALID, "char_width must be 1, 2 or 4");
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    RefStage add(s->book, OpenGenome::FOLD);
    const bool ok = add.contig(s->P, length);
    add.commit(s->book, [&] { if (ok) s->pending.append(data, char_width, length); });
    if (added) *added = ok ? 1 : 0;
  });
}
struct fa_fasta { FastaFile f; };
int fa_fasta_open(const char *path, fa_fasta **out) {
  return guarded([&] {
    FA_REQUIRE(path && out, FA_ERR_INVALID, "null argument");
    std::unique_ptr<fa_fasta> h(new fa_fasta());
    h->f.open(path);
    *out = h.release();
  });
}
int fa_fasta_next(fa_fasta *f, int *has_record, const char **id, int64_t *id_length, const unsigned char **seq, int64_t *seq_length) {
  return guarded([&] {
    const bool ok = f->f.next();
    *has_record = ok ? 1 : 0;
    if (!ok) return;
    *id = f->f.id.data(); *id_length = (int64_t)f->f.id.size();
    *seq = f->f.seq.data(); *seq_length = (int64_t)f->f.seq.size();
  });
}
void fa_fasta_close(fa_fasta *f) { delete f; }

int fa_sketch_add_fasta(fa_sketch *s, const char *path, int64_t *n_records, int64_t *n_short) {
  return guarded([&] {
    FA_REQUIRE(path, FA_ERR_INVALID, "null path");
    std::vector<FastaSeq> seqs;
    read_fasta_records(path, seqs);
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    std::vector<const void *> ptrs;
    std::vector<int64_t> all, lens;
    for (auto &q : seqs) all.push_back((int64_t)q.size);
    RefStage add(s->book, OpenGenome::FOLD);
    add.genomes(s->P, all.data(), nullptr, (int64_t)all.size(), 1, [&](int64_t c) { ptrs.push_back(seqs[(size_t)c].data.get()); lens.push_back(all[(size_t)c]); });
    add.commit(s->book, [&] { if (!ptrs.empty()) s->pending.append_many(ptrs.data(), lens.data(), (int64_t)ptrs.size(), 1); });
    if (n_records) *n_records = (int64_t)seqs.size();
    if (n_short) *n_short = add.n_short[0];
  });
}
// Many reference genomes at once from host buffers: contig c belongs to genome contig_genome[c] (non-decreasing); the effect of
// n_genomes x (fa_sketch_add_contig per contig, fa_sketch_end_genome) with ONE call of the packer over all contigs -- the
// per-genome calls wake the host pool a thousand times for a thousand genomes (0.4-0.5 s of `host_pack_s` on config 3).
int fa_sketch_add_genomes(fa_sketch *s, const void *const *contigs, const int64_t *lengths, const int32_t *contig_genome, int64_t n_contigs,
                          int32_t n_genomes, int char_width, int32_t *n_short) {
  return guarded([&] {
    FA_REQUIRE(char_width == 1 || char_width == 2 || char_width == 4, FA_ERR_INVALID, "char_width must be 1, 2 or 4");
    FA_REQUIRE(n_contigs >= 0 && n_genomes >= 0 && (n_contigs == 0 || (contigs && lengths && contig_genome)), FA_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    std::vector<const void *> ptrs;
    std::vector<int64_t> lens;
    RefStage add(s->book, OpenGenome::REFUSE, n_genomes);
    add.genomes(s->P, lengths, contig_genome, n_contigs, n_genomes, [&](int64_t c) { ptrs.push_back(contigs[c]); lens.push_back(lengths[c]); });
    add.commit(s->book, [&] { if (!ptrs.empty()) s->pending.append_many(ptrs.data(), lens.data(), (int64_t)ptrs.size(), char_width); });
    if (n_short) for (int32_t i = 0; i < n_genomes; i++) n_short[i] = (int32_t)add.n_short[(size_t)i];
  });
}
// Many reference genomes at once, one per FASTA file, in the order given: the files are read and packed concurrently (one
// task per file), then appended to the pending store exactly as fa_sketch_add_fasta would have added them one by one.
int fa_sketch_add_fasta_many(fa_sketch *s, const char *const *paths, int32_t n_paths, int64_t *n_records, int64_t *n_short) {
  return guarded([&] {
    FA_REQUIRE(paths && n_paths >= 0, FA_ERR_INVALID, "null paths or negative count");
    StageTrace tr("add_fasta_many");
    std::vector<PackedFasta> files;
    read_fasta_packed_many(paths, (size_t)n_paths, s->P.alphabet_size != 4, files);
    tr.mark("read_pack", nullptr);
    if (tr.on) {
      FastaTaskClock &c = fasta_task_clock();
      fprintf(stderr, "[fa trace] fasta tasks so far: %llu files, per-task sums: read %.1f ms, record search %.1f ms, pack %.1f ms\n", (unsigned long long)c.files.load(),
              c.read_ns.load() * 1e-6, c.scan_ns.load() * 1e-6, c.pack_ns.load() * 1e-6);
    }
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    tr.mark("bookkeeping", nullptr);
    sketch_add_packed_files(s, files.data(), n_paths, n_records, n_short);
    tr.mark("place", nullptr);
  });
}
// ---- files packed once, used many times (fa_packed) ----
int fa_packed_read(const char *const *paths, int32_t n_paths, int protein, fa_packed **out) {
  return guarded([&] {
    FA_REQUIRE(paths && out && n_paths >= 0, FA_ERR_INVALID, "null argument or negative count");
    std::unique_ptr<fa_packed> p(new fa_packed());
    p->protein = protein != 0;
    read_fasta_packed_many(paths, (size_t)n_paths, p->protein, p->files);
    *out = p.release();
  });
}
// more files behind the ones the set holds (read + packed concurrently, like fa_packed_read); all or nothing
int fa_packed_append(fa_packed *p, const char *const *paths, int32_t n_paths) {
  return guarded([&] {
    FA_REQUIRE(p && paths && n_paths >= 0, FA_ERR_INVALID, "null argument or negative count");
    std::vector<PackedFasta> more;
    read_fasta_packed_many(paths, (size_t)n_paths, p->protein, more);
    std::unique_lock<std::shared_mutex> grow(p->mtx);
    p->files.reserve(p->files.size() + more.size());
    for (auto &f : more) p->files.push_back(std::move(f));
  });
}
void fa_packed_free(fa_packed *p) { delete p; }
int fa_packed_info(fa_packed *p, int32_t *n_files, uint64_t *file_bytes, int64_t *records, int64_t *bases) {
  return guarded([&] {
    std::shared_lock<std::shared_mutex> hold(p->mtx);
    if (n_files) *n_files = (int32_t)p->files.size();
    for (size_t i = 0; i < p->files.size(); i++) {
      if (file_bytes) file_bytes[i] = (uint64_t)p->files[i].file_bytes;
      if (records) records[i] = (int64_t)p->files[i].rec_len.size();
      if (bases) { int64_t b = 0; for (int64_t l : p->files[i].rec_len) b += l; bases[i] = b; }
    }
  });
}
int fa_sketch_add_packed(fa_sketch *s, fa_packed *p, int32_t first, int32_t count, int64_t *n_records, int64_t *n_short) {
  return guarded([&] {
    FA_REQUIRE(p, FA_ERR_INVALID, "null packed set");
    std::shared_lock<std::shared_mutex> hold(p->mtx);
    FA_REQUIRE(first >= 0 && count >= 0 && (size_t)first + (size_t)count <= p->files.size(), FA_ERR_INVALID, "file range outside the packed set");
    FA_REQUIRE(p->protein == (s->P.alphabet_size != 4), FA_ERR_INVALID, "the files were packed for the other alphabet");
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    sketch_add_packed_files(s, p->files.data() + first, count, n_records, n_short);
  });
}
int fa_genomes_reload_packed(fa_mapper *m, fa_genomes *g, fa_packed *p, int32_t first, int32_t count) {
  return guarded([&] {
    FA_REQUIRE(g && p, FA_ERR_INVALID, "null argument");
    std::shared_lock<std::shared_mutex> hold(p->mtx);
    FA_REQUIRE(first >= 0 && count >= 0 && (size_t)first + (size_t)count <= p->files.size(), FA_ERR_INVALID, "file range outside the packed set");
    FA_REQUIRE(p->protein == (m->P.alphabet_size != 4), FA_ERR_INVALID, "the files were packed for the other alphabet");
    try { fill_genomes_from_packed(m, g, p->files.data() + first, count, true); } catch (...) { g->reset_empty(); throw; }
  });
}
int fa_sketch_end_genome(fa_sketch *s) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    RefStage add(s->book, OpenGenome::FOLD);
    add.end_genome();
    add.commit(s->book);
  });
}
int fa_sketch_abort_genome(fa_sketch *s) {
  return guarded([&] { std::lock_guard<std::mutex> lock(s->mtx); s->book.cur_total = 0; });
}
int fa_sketch_clear(fa_sketch *s) {
  return guarded([&] { std::lock_guard<std::mutex> lock(s->mtx); s->reset_data(); });
}
int fa_sketch_num_minimizers(fa_sketch *s, int64_t *n) {
  return guarded([&] { std::lock_guard<std::mutex> lock(s->mtx); s->flush(); *n = s->nrec; });
}
int fa_sketch_get_minimizers(fa_sketch *s, uint32_t *hash, int32_t *seq_id, int32_t *wpos) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    s->flush();
    if (s->nrec == 0) return;
    s->rec.store(hash, seq_id, wpos, (size_t)s->nrec, hipMemcpyDeviceToHost, s->stream);
    FA_HIP(hipStreamSynchronize(s->stream));
  });
}
int fa_sketch_num_genomes(fa_sketch *s, int64_t *n) {
  return guarded([&] { *n = (int64_t)s->book.lengths.size(); });
}
int fa_sketch_get_state(fa_sketch *s, uint64_t *lengths, int32_t *sbf, int64_t *counter) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    for (size_t i = 0; i < s->book.lengths.size(); i++) { lengths[i] = s->book.lengths[i]; sbf[i] = s->book.seqs_by_file[i]; }
    *counter = s->book.counter;
  });
}
// the saved state of a sketch replaces its content; the records come from host (hipMemcpyHostToDevice) or device memory
static int sketch_set_state(fa_sketch *s, int64_t n_genomes, const uint64_t *lengths, const int32_t *sbf, int64_t counter, int64_t n_min,
                            const uint32_t *hash, const int32_t *seq_id, const int32_t *wpos, hipMemcpyKind kind) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    FA_REQUIRE(n_min >= 0 && n_genomes >= 0, FA_ERR_INVALID, "negative count");
    s->reset_data();
    s->book.lengths.assign(lengths, lengths + n_genomes);
    s->book.seqs_by_file.assign(sbf, sbf + n_genomes);
    s->book.counter = counter;
    if (n_min > 0) {
      require_device();
      bind_device(s->device);
      if (!s->stream) FA_HIP(hipStreamCreate(&s->stream));
      s->rec.load(hash, seq_id, wpos, (size_t)n_min, kind, s->stream);
      FA_HIP(hipStreamSynchronize(s->stream));
    }
    s->nrec = n_min;
  });
}
int fa_sketch_set_state(fa_sketch *s, int64_t n_genomes, const uint64_t *lengths, const int32_t *sbf, int64_t counter,
                        int64_t n_min, const uint32_t *hash, const int32_t *seq_id, const int32_t *wpos) {
  return sketch_set_state(s, n_genomes, lengths, sbf, counter, n_min, hash, seq_id, wpos, hipMemcpyHostToDevice);
}

// Device-pointer variants of the two calls above: the minimizer records never leave HBM.  Used by the multi-GPU index
// build (every rank sketches a share of the references, the shards are all-gathered over RCCL into
// tensors the caller owns, and every rank loads the merged records).  The caller synchronises its own stream before
// the call; the library synchronises its stream before returning.
int fa_sketch_get_minimizers_device(fa_sketch *s, int64_t cap, uint32_t *d_hash, int32_t *d_seq_id, int32_t *d_wpos) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    s->flush();
    FA_REQUIRE(cap >= s->nrec, FA_ERR_INVALID, "destination holds fewer records than the sketch");
    if (s->nrec == 0) return;
    s->rec.store(d_hash, d_seq_id, d_wpos, (size_t)s->nrec, hipMemcpyDeviceToDevice, s->stream);
    FA_HIP(hipStreamSynchronize(s->stream));
  });
}
int fa_sketch_set_state_device(fa_sketch *s, int64_t n_genomes, const uint64_t *lengths, const int32_t *sbf, int64_t counter,
                               int64_t n_min, const uint32_t *d_hash, const int32_t *d_seq_id, const int32_t *d_wpos) {
  return sketch_set_state(s, n_genomes, lengths, sbf, counter, n_min, d_hash, d_seq_id, d_wpos, hipMemcpyDeviceToDevice);
}

// A subset of the genomes as a sketch of its own, and the frequency filter an index of the sketch would have: what maps a
// collection group by group out of one resident sketch (fa_select.hip.h has the semantics and the road).  Both run on the
// sketch's stream and have finished when they return.
int fa_sketch_select(fa_sketch *s, const int32_t *genomes, int32_t n, fa_sketch **out) {
  return guarded([&] {
    FA_REQUIRE(s && out && n >= 0 && (genomes || n == 0), FA_ERR_INVALID, "null sketch, list or destination, or a negative count");
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    const RefBook &book = s->book;
    const int64_t G = (int64_t)book.lengths.size();
    FA_REQUIRE(book.counter == (G ? (int64_t)book.seqs_by_file.back() : 0), FA_ERR_INVALID, "a genome is still open (add_contig without end_genome)");
    for (int32_t i = 0; i < n; i++) {
      FA_REQUIRE(genomes[i] >= 0 && genomes[i] < G, FA_ERR_INVALID, "a selected genome is outside [0, n_genomes)");
      FA_REQUIRE(i == 0 || genomes[i] > genomes[i - 1], FA_ERR_INVALID, "the selected genomes must ascend strictly");
    }
    require_device();
    s->flush();
    bind_device(s->device);
    struct Free { void operator()(fa_sketch *p) const { fa_sketch_free(p); } };
    std::unique_ptr<fa_sketch, Free> o(new fa_sketch());
    o->P = s->P;
    o->device = s->device;
    o->reset_data();
    // one segment per selected genome: its contig range in the source and what its contig ids move by
    std::vector<int32_t> contig_lo((size_t)n), contig_hi((size_t)n), delta((size_t)n);
    int32_t contigs = 0;
    for (int32_t i = 0; i < n; i++) {
      const int32_t g = genomes[i];
      contig_lo[(size_t)i] = g ? book.seqs_by_file[(size_t)g - 1] : 0;
      contig_hi[(size_t)i] = book.seqs_by_file[(size_t)g];
      delta[(size_t)i] = contigs - contig_lo[(size_t)i];
      contigs += contig_hi[(size_t)i] - contig_lo[(size_t)i];
      o->book.lengths.push_back(book.lengths[(size_t)g]);
      o->book.seqs_by_file.push_back(contigs);
    }
    o->book.counter = contigs;
    if (n > 0 && s->nrec > 0) {
      require_device();
      if (!s->stream) FA_HIP(hipStreamCreate(&s->stream));
      hipStream_t st = s->stream;
      DevBuf<int32_t> d_contig_lo, d_contig_hi, d_delta;
      DevBuf<int64_t> d_rec, d_off;                             // d_rec: [n] first records, then [n] ends
      d_contig_lo.upload(contig_lo, st); d_contig_hi.upload(contig_hi, st);
      d_rec.ensure(2 * (size_t)n);
      hipLaunchKernelGGL(k_select_bounds, dim3(ceil_div(2 * (int64_t)n, 256)), dim3(256), 0, st, s->rec.seq.p, s->nrec, d_contig_lo.p, d_contig_hi.p, n,
                         d_rec.p, d_rec.p + n);
      FA_HIP(hipGetLastError());
      std::vector<int64_t> rec(2 * (size_t)n), off((size_t)n + 1);
      d_rec.download(rec.data(), rec.size(), st);
      FA_HIP(hipStreamSynchronize(st));
      int64_t total = 0;
      for (int32_t i = 0; i < n; i++) {
        const int64_t lo = rec[(size_t)i], hi = rec[(size_t)n + (size_t)i];
        FA_REQUIRE(0 <= lo && lo <= hi && hi <= s->nrec, FA_ERR_INTERNAL, "the records of the sketch are not sorted by contig id");
        off[(size_t)i] = total;
        total += hi - lo;
      }
      off[(size_t)n] = total;
      if (total > 0) {
        o->rec.hash.ensure((size_t)total); o->rec.seq.ensure((size_t)total); o->rec.wpos.ensure((size_t)total);
        d_off.upload(off, st); d_delta.upload(delta, st);
        SelectArgs a;
        a.src_hash = s->rec.hash.p; a.src_seq = s->rec.seq.p; a.src_wpos = s->rec.wpos.p;
        a.dst_hash = o->rec.hash.p; a.dst_seq = o->rec.seq.p; a.dst_wpos = o->rec.wpos.p;
        a.dst_off = d_off.p; a.src_lo = d_rec.p; a.delta = d_delta.p; a.n = n; a.total = total;
        const int64_t tiles = (total + SEL_TILE - 1) / SEL_TILE;
        hipLaunchKernelGGL(k_select_copy, dim3((unsigned)std::min<int64_t>(tiles, SEL_MAX_BLOCKS)), dim3(SEL_THREADS), 0, st, a);
        FA_HIP(hipGetLastError());
        FA_HIP(hipStreamSynchronize(st));
      }
      o->nrec = total;
    }
    *out = o.release();
  });
}

int fa_sketch_frequency(fa_sketch *s, int *threshold, int64_t cap, uint32_t *d_drop_keys, int64_t *n_drop) {
  return guarded([&] {
    FA_REQUIRE(s && threshold && n_drop && cap >= 0 && (d_drop_keys || cap == 0), FA_ERR_INVALID, "null sketch or destination, or a negative capacity");
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    require_device();
    s->flush();
    bind_device(s->device);
    const int64_t N = s->nrec;
    // (the list lengths are uint32, as in the index; nothing here is a record NUMBER, so 2^31 is no bound)
    FA_REQUIRE(N <= (int64_t)UINT32_MAX, FA_ERR_UNSUPPORTED, "more than 2^32 - 1 minimizers in one sketch");
    int thr = INT_MAX;
    int64_t dropped = 0;
    DevBuf<uint32_t> sorted_hash, uniq, counts, num_runs;
    if (N > 0) {
      if (!s->stream) FA_HIP(hipStreamCreate(&s->stream));
      hipStream_t st = s->stream;
      DevBuf<unsigned char> temp;
      DevBuf<size_t> n_selected;
      sorted_hash.ensure((size_t)N); uniq.ensure((size_t)N); counts.ensure((size_t)N); num_runs.ensure(1); n_selected.ensure(1);
      with_temp(temp, [&](void *t, size_t &bytes) { return rocprim::radix_sort_keys(t, bytes, s->rec.hash.p, sorted_hash.p, (size_t)N, 0u, 32u, st); });
      with_temp(temp, [&](void *t, size_t &bytes) {
        return rocprim::run_length_encode(t, bytes, sorted_hash.p, (size_t)N, uniq.p, counts.p, num_runs.p, st);
      });
      uint32_t U = 0;
      num_runs.download(&U, 1, st);
      FA_HIP(hipStreamSynchronize(st));
      thr = frequency_threshold(counts.p, (int64_t)U, temp, st);
      if (thr < INT_MAX) {
        // the distinct hashes ascend, and so do the ones kept; the sorted copy has served and takes them
        with_temp(temp, [&](void *t, size_t &bytes) {
          return rocprim::select(t, bytes, uniq.p, rocprim::make_transform_iterator(counts.p, ListAtLeast{(uint32_t)thr}), sorted_hash.p, n_selected.p,
                                 (size_t)U, st);
        });
        size_t kept = 0;
        n_selected.download(&kept, 1, st);
        FA_HIP(hipStreamSynchronize(st));
        dropped = (int64_t)kept;
      }
      if (dropped > cap) {
        *n_drop = dropped;
        FA_REQUIRE(false, FA_ERR_INVALID, "destination holds fewer keys than reach the threshold (*n_drop is what it takes)");
      }
      if (dropped > 0) {
        FA_HIP(hipMemcpyAsync(d_drop_keys, sorted_hash.p, (size_t)dropped * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        FA_HIP(hipStreamSynchronize(st));
      }
    }
    *threshold = thr;
    *n_drop = dropped;
  });
}

int fa_sketch_index(fa_sketch *s, fa_mapper **out) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    require_device();
    s->flush();
    bind_device(s->device);
    std::unique_ptr<fa_mapper> m(new fa_mapper());
    m->P = s->P;
    m->device = s->device;
    if (m->device < 0) FA_HIP(hipGetDevice(&m->device));
    FA_HIP(hipStreamCreate(&m->stream));
    m->N = s->nrec;
    s->rec.reserve((size_t)m->N + 4, (size_t)m->N, m->stream);
    m->rec_hash = std::move(s->rec.hash); m->rec_seq = std::move(s->rec.seq); m->rec_wpos = std::move(s->rec.wpos);
    m->lengths = s->book.lengths;
    m->seqs_by_file = s->book.seqs_by_file;
    if (!m->seqs_by_file.empty() && m->seqs_by_file.back() < (int32_t)s->book.counter) {
      // contigs added after the last end_genome belong to no genome; keep the tables consistent
      m->seqs_by_file.back() = (int32_t)s->book.counter;
    }
    build_index(*m);
    s->reset_data();                                     // _fastani.pyx:803-804
    *out = m.release();
  });
}

void fa_mapper_free(fa_mapper *m) {
  if (!m) return;
  if (m->stream) (void)hipStreamDestroy(m->stream);
  delete m;   // the workspaces release their own streams, events and pinned blocks
}
int fa_mapper_freq_threshold(fa_mapper *m, int *thr) { *thr = m->freq_threshold; return FA_OK; }
int fa_mapper_lookup_size(fa_mapper *m, int64_t *n) { *n = m->U; return FA_OK; }
int fa_mapper_device(fa_mapper *m, int *device) { *device = m->device; return FA_OK; }
int fa_mapper_lookup_export_device(fa_mapper *m, int64_t cap, uint32_t *d_keys, int32_t *d_counts) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    FA_REQUIRE(cap >= m->U, FA_ERR_INVALID, "destination smaller than the lookup index");
    if (m->U == 0) return;
    FA_HIP(hipMemcpyAsync(d_keys, m->uniq_hash.p, (size_t)m->U * sizeof(uint32_t), hipMemcpyDeviceToDevice, m->stream));
    hipLaunchKernelGGL(k_list_lengths, dim3(ceil_div(m->U, 256)), dim3(256), 0, m->stream, m->uniq_off.p, (int64_t)m->U, d_counts);
    FA_HIP(hipGetLastError());
    FA_HIP(hipStreamSynchronize(m->stream));
  });
}
int fa_mapper_set_global_frequency(fa_mapper *m, int threshold, int64_t n_drop, const uint32_t *d_drop_keys) {
  return guarded([&] {
    FA_REQUIRE(threshold >= 0 && n_drop >= 0, FA_ERR_INVALID, "negative threshold or key count");
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    m->freq_threshold = threshold;
    if (n_drop > 0 && m->U > 0) {
      hipLaunchKernelGGL(k_drop_keys, dim3(ceil_div(n_drop, 256)), dim3(256), 0, m->stream, d_drop_keys, n_drop, m->table_bits, m->table.p);
      FA_HIP(hipGetLastError());
    }
    FA_HIP(hipStreamSynchronize(m->stream));
  });
}
int fa_mapper_lookup_keys(fa_mapper *m, uint32_t *keys) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    m->uniq_hash.download(keys, (size_t)m->U, m->stream);
    FA_HIP(hipStreamSynchronize(m->stream));
  });
}
static int64_t host_find(fa_mapper *m, uint32_t hash, uint32_t *off, uint32_t *cnt) {
  // binary search with single-element reads (introspection path, not performance critical)
  int64_t lo = 0, hi = m->U;
  while (lo < hi) {
    int64_t mid = (lo + hi) / 2;
    uint32_t v;
    FA_HIP(hipMemcpy(&v, m->uniq_hash.p + mid, 4, hipMemcpyDeviceToHost));
    if (v < hash) lo = mid + 1; else hi = mid;
  }
  if (lo >= m->U) return -1;
  uint32_t v, o[2];
  FA_HIP(hipMemcpy(&v, m->uniq_hash.p + lo, 4, hipMemcpyDeviceToHost));
  if (v != hash) return -1;
  FA_HIP(hipMemcpy(o, m->uniq_off.p + lo, 8, hipMemcpyDeviceToHost));
  *off = o[0]; *cnt = o[1] - o[0];
  return lo;
}
int fa_mapper_lookup_count(fa_mapper *m, uint32_t hash, int64_t *count) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    uint32_t off, cnt;
    *count = host_find(m, hash, &off, &cnt) < 0 ? -1 : (int64_t)cnt;
  });
}
int fa_mapper_lookup_get(fa_mapper *m, uint32_t hash, int32_t *seq_id, int32_t *wpos, int64_t cap) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    uint32_t off, cnt;
    FA_REQUIRE(host_find(m, hash, &off, &cnt) >= 0, FA_ERR_INVALID, "hash not in the lookup index");
    std::vector<uint32_t> ridx(cnt);
    FA_HIP(hipMemcpy(ridx.data(), m->pos_ridx.p + off, (size_t)cnt * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < cnt && (int64_t)i < cap; i++) {
      FA_HIP(hipMemcpy(&seq_id[i], m->rec_seq.p + ridx[i], 4, hipMemcpyDeviceToHost));
      FA_HIP(hipMemcpy(&wpos[i], m->rec_wpos.p + ridx[i], 4, hipMemcpyDeviceToHost));
    }
  });
}
int fa_mapper_num_minimizers(fa_mapper *m, int64_t *n) { *n = m->N; return FA_OK; }
int fa_mapper_get_minimizers(fa_mapper *m, uint32_t *hash, int32_t *seq_id, int32_t *wpos) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    if (m->N == 0) return;
    m->rec_hash.download(hash, (size_t)m->N, m->stream);
    m->rec_seq.download(seq_id, (size_t)m->N, m->stream);
    m->rec_wpos.download(wpos, (size_t)m->N, m->stream);
    FA_HIP(hipStreamSynchronize(m->stream));
  });
}
int fa_mapper_num_genomes(fa_mapper *m, int64_t *n) { *n = (int64_t)m->lengths.size(); return FA_OK; }
int fa_mapper_get_state(fa_mapper *m, uint64_t *lengths, int32_t *sbf) {
  for (size_t i = 0; i < m->lengths.size(); i++) { lengths[i] = m->lengths[i]; sbf[i] = m->seqs_by_file[i]; }
  return FA_OK;
}

int fa_genomes_upload(fa_mapper *m, const void *const *contigs, const int64_t *lengths, const int32_t *contig_genome,
                      int64_t n_contigs, int32_t n_genomes, int char_width, fa_genomes **out) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    auto g = std::make_unique<fa_genomes>();
    fill_genomes(g.get(), m->P, m->stream, contigs, lengths, contig_genome, n_contigs, n_genomes, char_width, nullptr, nullptr, nullptr, false);
    *out = g.release();
  });
}
int fa_genomes_upload_fasta(fa_mapper *m, const char *const *paths, int32_t n_paths, fa_genomes **out) {
  return guarded([&] {
    FA_REQUIRE(n_paths >= 0, FA_ERR_INVALID, "negative count");
    std::unique_ptr<fa_genomes> g(new fa_genomes());
    fill_genomes_from_fasta(m, g.get(), paths, n_paths, false);
    *out = g.release();
  });
}
int fa_genomes_reload_fasta(fa_mapper *m, fa_genomes *g, const char *const *paths, int32_t n_paths) {
  return guarded([&] {
    FA_REQUIRE(g && n_paths >= 0, FA_ERR_INVALID, "null batch or negative count");
    try { fill_genomes_from_fasta(m, g, paths, n_paths, true); } catch (...) { g->reset_empty(); throw; }
  });
}
void fa_genomes_free(fa_genomes *g) { delete g; }
int fa_genomes_info(fa_genomes *g, int32_t *n_genomes, uint64_t *tf, uint64_t *tl, int32_t *ns) {
  if (n_genomes) *n_genomes = g->n_genomes;
  for (int i = 0; i < g->n_genomes; i++) {
    if (tf) tf[i] = g->total_fragments[i];
    if (tl) tl[i] = g->total_length[i];
    if (ns) ns[i] = g->n_short[i];
  }
  return FA_OK;
}
int fa_mapper_query_genomes(fa_mapper *m, fa_genomes *g, int32_t first, int32_t count, fa_cgi_row *rows, int64_t cap,
                            int64_t *n_rows, int rows_device) {
  return guarded([&] {
    WorkspaceLease lease(*m);
    *n_rows = run_query(*m, *lease.w, *g, first, count, rows, cap, rows_device != 0);
  });
}
int fa_mapper_query_genomes_mappings(fa_mapper *m, fa_genomes *g, int32_t first, int32_t count, fa_cgi_row *rows, int64_t cap,
                                     int64_t *n_rows, int rows_device, fa_hit_mapping *maps, int64_t map_cap, int64_t *n_maps,
                                     int maps_device) {
  return guarded([&] {
    WorkspaceLease lease(*m);
    const MapRequest want{maps, map_cap, n_maps, maps_device != 0};
    *n_rows = run_query(*m, *lease.w, *g, first, count, rows, cap, rows_device != 0, &want);
  });
}
int fa_mapper_query_genomes_mappings_stream(fa_mapper *m, fa_genomes *g, int32_t first, int32_t count, fa_cgi_row *rows, int64_t cap,
                                            int64_t *n_rows, int rows_device, fa_mapping_sink sink, void *user, int64_t *n_maps) {
  return guarded([&] {
    WorkspaceLease lease(*m);
    MapRequest want{nullptr, 0, n_maps, false};
    want.stream = true; want.fn = sink; want.user = user;
    *n_rows = run_query(*m, *lease.w, *g, first, count, rows, cap, rows_device != 0, &want);
  });
}
int fa_table_pairs(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes, const uint64_t *query_lengths,
                   const uint64_t *reference_lengths, const fa_table_params *p, fa_pair *pairs, int64_t cap, int64_t *n_pairs,
                   int pairs_device) {
  return guarded([&] {
    TableRequest want;
    want.pairs = pairs; want.cap = cap; want.n_pairs = n_pairs; want.pairs_device = pairs_device != 0;
    table_reduce(rows, n_rows, rows_device != 0, n_genomes, query_lengths, reference_lengths, p, want);
  });
}
int fa_table_clusters(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes, const uint64_t *query_lengths,
                      const uint64_t *reference_lengths, const fa_table_params *p, int32_t *labels, int labels_device,
                      int32_t *n_clusters, int64_t *stats) {
  return guarded([&] {
    TableRequest want;
    want.clusters = true;
    want.labels = labels; want.labels_device = labels_device != 0; want.n_clusters = n_clusters; want.stats = stats;
    table_reduce(rows, n_rows, rows_device != 0, n_genomes, query_lengths, reference_lengths, p, want);
  });
}
int fa_table_representatives(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes, const uint64_t *query_lengths,
                             const uint64_t *reference_lengths, const fa_table_params *p, const int32_t *order, int32_t *labels,
                             double *identity, int out_device, int32_t *n_representatives, int64_t *stats) {
  return guarded([&] {
    TableRequest want;
    want.clusters = want.representatives = true;
    want.order = order; want.labels = labels; want.identity = identity; want.labels_device = out_device != 0;
    want.n_clusters = n_representatives; want.stats = stats;
    table_reduce(rows, n_rows, rows_device != 0, n_genomes, query_lengths, reference_lengths, p, want);
  });
}
int fa_table_best(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_queries, int32_t n_references,
                  const uint64_t *query_lengths, const uint64_t *reference_lengths, const fa_best_params *p, fa_cgi_row *best,
                  int64_t *offsets, int64_t cap, int64_t *n_best, int out_device, int64_t *stats) {
  return guarded([&] {
    table_best(rows, n_rows, rows_device != 0, n_queries, n_references, query_lengths, reference_lengths, p, best, offsets, cap, n_best,
               out_device != 0, stats);
  });
}
int fa_screen_tile(int32_t s, int32_t *tile) {
  return guarded([&] {
    FA_REQUIRE(tile && s >= 1 && s <= SCR_MAX_S, FA_ERR_INVALID, "the signature size must be in [1, 4096]");
    *tile = screen_tile(s);
  });
}
int fa_screen_signatures(const uint32_t *d_hash, const int32_t *d_seq_id, int64_t n_records, const int32_t *sbf, int32_t n_genomes,
                         int32_t s, uint32_t *d_sig, int32_t *d_count) {
  return guarded([&] { screen_signatures(d_hash, d_seq_id, n_records, sbf, n_genomes, s, d_sig, d_count); });
}
int fa_screen_pairs(const uint32_t *d_sig_a, const int32_t *d_count_a, int32_t n_a, const uint32_t *d_sig_b, const int32_t *d_count_b,
                    int32_t n_b, int32_t s, int triangular, int32_t jn, int32_t jd, fa_screen_pair *pairs, int64_t cap, int64_t *n_pairs,
                    int pairs_device, int64_t *stats) {
  return guarded([&] {
    screen_pairs(d_sig_a, d_count_a, n_a, d_sig_b, d_count_b, n_b, s, triangular != 0, jn, jd, pairs, cap, n_pairs, pairs_device != 0, stats);
  });
}
int fa_screen_groups(const fa_screen_pair *pairs, int64_t n_pairs, int pairs_device, int32_t n_genomes, int32_t *labels, int labels_device,
                     int32_t *n_groups) {
  return guarded([&] { screen_groups(pairs, n_pairs, pairs_device != 0, n_genomes, labels, labels_device != 0, n_groups); });
}
int fa_mapper_set_mapping_stage(fa_mapper *m, int64_t records) {
  return guarded([&] {
    FA_REQUIRE(m && records >= 1, FA_ERR_INVALID, "the mapping stage holds at least one record");
    std::lock_guard<std::mutex> lock(m->mtx);
    m->map_stage = records;
  });
}
int fa_rules_default(fa_rules *out) {
  return guarded([&] { FA_REQUIRE(out, FA_ERR_INVALID, "null destination"); *out = default_rules(); });
}
static void validate_rules(const fa_rules &r) {
  FA_REQUIRE(r.l2_confidence > 0.0f && r.l2_confidence < 1.0f, FA_ERR_INVALID, "l2_confidence must lie strictly inside (0, 1)");
  FA_REQUIRE(r.slide_end == 0 || r.slide_end == 1, FA_ERR_INVALID, "slide_end must be 0 (windows) or 1 (fragment)");
  FA_REQUIRE(r.cgi_ties == 0 || r.cgi_ties == 1, FA_ERR_INVALID, "cgi_ties must be 0 (smallest) or 1 (largest)");
}
// The interval only feeds the pass table (StatTables::pass_shared): it is rebuilt and uploaded, and the table it replaces is
// retired like the generations ensure_luts outgrows -- calls in flight read it to their end.  The other two rules are argument
// words of the kernels of the calls that start from now on.
int fa_mapper_set_rules(fa_mapper *m, const fa_rules *r) {
  return guarded([&] {
    FA_REQUIRE(r, FA_ERR_INVALID, "null rules");
    validate_rules(*r);
    FA_REQUIRE(m, FA_ERR_INVALID, "null mapper");
    std::lock_guard<std::mutex> lock(m->mtx);
    if (same_rules(m->rules, *r)) return;
    if (r->l2_confidence != m->stats.ci) {
      StatTables next = m->stats;                            // (a failed upload leaves the mapper as it was)
      next.set_ci(r->l2_confidence);
      if (m->d_pass.p) {
        bind_device(m->device);
        DevBuf<int32_t> d_next;
        d_next.upload(next.pass_shared, m->stream);
        FA_HIP(hipStreamSynchronize(m->stream));
        m->retired_i32.push_back(std::move(m->d_pass));
        m->d_pass = std::move(d_next);
      }
      m->stats = std::move(next);
    }
    m->rules = *r;
  });
}
int fa_mapper_get_rules(fa_mapper *m, fa_rules *out) {
  return guarded([&] {
    FA_REQUIRE(m && out, FA_ERR_INVALID, "null mapper or destination");
    std::lock_guard<std::mutex> lock(m->mtx);
    *out = m->rules;
  });
}
int fa_pass_threshold(int sketch_size, int k, float identity, float ci, int *min_shared) {
  return guarded([&] {
    FA_REQUIRE(min_shared && sketch_size > 0 && k >= 1, FA_ERR_INVALID, "sketch_size and k must be positive");
    FA_REQUIRE(ci > 0.0f && ci < 1.0f, FA_ERR_INVALID, "the confidence interval must lie strictly inside (0, 1)");
    *min_shared = stat_pass_threshold(sketch_size, k, identity, ci);
  });
}
int fa_mapper_mapping_memory(fa_mapper *m, int64_t out[4]) {
  return guarded([&] {
    FA_REQUIRE(m && out, FA_ERR_INVALID, "null mapper or destination");
    std::lock_guard<std::mutex> lock(m->mtx);
    for (int i = 0; i < 4; i++) out[i] = 0;
    if (m->last_map_ws < 0) return;
    const Workspace &w = m->ws[m->last_map_ws];
    out[0] = w.map_stage.records;
    out[1] = out[2] = (int64_t)w.map_stage.bytes();
    out[3] = (int64_t)w.winners.block;
  });
}
static int query_one(fa_mapper *m, const void *const *contigs, const int64_t *lengths, int n_contigs, int char_width,
                     fa_cgi_row *rows, int64_t cap, int64_t *n_rows, int *n_short, uint64_t *total_fragments,
                     uint64_t *total_length, const MapRequest *want) {
  return guarded([&] {
    WorkspaceLease lease(*m);
    std::vector<int32_t> cg((size_t)std::max(n_contigs, 1), 0);
    float host_ms[3] = {0, 0, 0};
    std::unique_ptr<fa_genomes> g = lease.w->query_batch ? std::move(lease.w->query_batch) : std::make_unique<fa_genomes>();
    fill_genomes(g.get(), m->P, lease.w->stream, contigs, lengths, cg.data(), n_contigs, 1, char_width, host_ms, &lease.w->pin_image, nullptr, false);
    if (n_short) *n_short = g->n_short[0];
    if (total_fragments) *total_fragments = g->total_fragments[0];
    if (total_length) *total_length = g->total_length[0];
    const auto t0 = std::chrono::steady_clock::now();
    *n_rows = run_query(*m, *lease.w, *g, 0, 1, rows, cap, false, want);
    // host-side split of the boundary call (wall clock): packing, fragment/tile tables, H2D, pass + rows D2H
    for (int i = 0; i < 3; i++) lease.w->last_ms[MS_HOST + i] = host_ms[i];
    lease.w->last_ms[MS_CALL] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    lease.w->last_genomes = nullptr;
    lease.w->query_batch = std::move(g);                 // keep the device buffers for the next call
  });
}
int fa_mapper_query(fa_mapper *m, const void *const *contigs, const int64_t *lengths, int n_contigs, int char_width,
                    fa_cgi_row *rows, int64_t cap, int64_t *n_rows, int *n_short, uint64_t *total_fragments,
                    uint64_t *total_length) {
  return query_one(m, contigs, lengths, n_contigs, char_width, rows, cap, n_rows, n_short, total_fragments, total_length, nullptr);
}
int fa_mapper_query_mappings(fa_mapper *m, const void *const *contigs, const int64_t *lengths, int n_contigs, int char_width,
                             fa_cgi_row *rows, int64_t cap, int64_t *n_rows, int *n_short, uint64_t *total_fragments,
                             uint64_t *total_length, fa_hit_mapping *maps, int64_t map_cap, int64_t *n_maps) {
  const MapRequest want{maps, map_cap, n_maps, false};
  return query_one(m, contigs, lengths, n_contigs, char_width, rows, cap, n_rows, n_short, total_fragments, total_length, &want);
}
int fa_mapper_query_mappings_stream(fa_mapper *m, const void *const *contigs, const int64_t *lengths, int n_contigs, int char_width,
                                    fa_cgi_row *rows, int64_t cap, int64_t *n_rows, int *n_short, uint64_t *total_fragments,
                                    uint64_t *total_length, fa_mapping_sink sink, void *user, int64_t *n_maps) {
  MapRequest want{nullptr, 0, n_maps, false};
  want.stream = true; want.fn = sink; want.user = user;
  return query_one(m, contigs, lengths, n_contigs, char_width, rows, cap, n_rows, n_short, total_fragments, total_length, &want);
}

// The workspace holds the intermediates of the last part it ran.  A pass that ran in more parts (several passes of one
// genome, or parts that were repeated) has left only its last part behind: say so instead of handing out a fraction of
// the pass as if it were all of it.  Returns whether the workspace holds a pass at all.
static bool holds_last_pass(const Workspace &w) {
  FA_REQUIRE(w.last_F == w.pass_F, FA_ERR_UNSUPPORTED,
             "the stage getters hold the last part of every lane only, and the last pass ran in more parts than that");
  return w.last_F > 0;
}
int fa_mapper_debug_mappings(fa_mapper *m, fa_mapping *out, int64_t cap, int64_t *n) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    Workspace &w = m->ws[m->last_ws];
    ensure_luts(*m, 1);
    int64_t k = 0;
    if (holds_last_pass(w)) {
      const uint32_t L = w.last_loci;
      std::vector<int32_t> lf(L), ls(L), lp(L), lsh(L), qs((size_t)w.last_F);
      size_t at = 0;
      for_each_locus_slice(w, [&](size_t first, size_t count) {
        FA_HIP(hipMemcpyAsync(lf.data() + at, w.l_frag.p + first, count * 4, hipMemcpyDeviceToHost, w.stream));
        FA_HIP(hipMemcpyAsync(ls.data() + at, w.l_seq.p + first, count * 4, hipMemcpyDeviceToHost, w.stream));
        FA_HIP(hipMemcpyAsync(lp.data() + at, w.l_pos.p + first, count * 4, hipMemcpyDeviceToHost, w.stream));
        FA_HIP(hipMemcpyAsync(lsh.data() + at, w.l_shared.p + first, count * 4, hipMemcpyDeviceToHost, w.stream));
        at += count;
      });
      w.q_size.download(qs.data(), (size_t)w.last_F, w.stream);
      FA_HIP(hipStreamSynchronize(w.stream));
      // (the filter of doL2Mapping at the interval the call ran with, which the mapper may have left since)
      std::vector<int32_t> own;
      if (w.rules.l2_confidence != m->stats.ci) {
        own.resize(m->stats.pass_shared.size());
        for (size_t s = 0; s < own.size(); s++) own[s] = stat_pass_threshold((int)s, m->stats.k, m->stats.pid, w.rules.l2_confidence);
      }
      const std::vector<int32_t> &pass_shared = own.empty() ? m->stats.pass_shared : own;
      for (uint32_t i = 0; i < L; i++) {
        int s = qs[lf[i]];
        if (lsh[i] < pass_shared[s]) continue;
        if (k < cap) {
          fa_mapping r;
          r.query_seq_id = lf[i]; r.ref_seq_id = ls[i]; r.ref_start_pos = lp[i]; r.sketch_size = s;
          r.conserved = lsh[i]; r.query_id = 0;
          out[k] = r;
        }
        k++;
      }
    }
    *n = k;
  });
}
int fa_mapper_debug_l1(fa_mapper *m, int32_t *frag, int32_t *seq_id, int32_t *rs, int32_t *re, int64_t cap, int64_t *n) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    Workspace &w = m->ws[m->last_ws];
    int64_t k = 0;
    if (holds_last_pass(w)) {
      for_each_locus_slice(w, [&](size_t first, size_t count) {
        const size_t c = (size_t)std::max<int64_t>(0, std::min<int64_t>((int64_t)count, cap - k));
        if (c) {
          FA_HIP(hipMemcpyAsync(frag + k, w.l_frag.p + first, c * 4, hipMemcpyDeviceToHost, w.stream));
          FA_HIP(hipMemcpyAsync(seq_id + k, w.l_seq.p + first, c * 4, hipMemcpyDeviceToHost, w.stream));
          FA_HIP(hipMemcpyAsync(rs + k, w.l_start.p + first, c * 4, hipMemcpyDeviceToHost, w.stream));
          FA_HIP(hipMemcpyAsync(re + k, w.l_end.p + first, c * 4, hipMemcpyDeviceToHost, w.stream));
        }
        k += (int64_t)count;
      });
      FA_HIP(hipStreamSynchronize(w.stream));
    }
    *n = k;
  });
}
int fa_mapper_debug_query_sketch(fa_mapper *m, int64_t fragment, uint32_t *hashes, int32_t cap, int32_t *sketch_size) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    Workspace &w = m->ws[m->last_ws];
    if (!holds_last_pass(w) || fragment < 0 || fragment >= w.last_F) throw Error(FA_ERR_INVALID, "fragment out of range");
    int32_t s = 0;
    FA_HIP(hipMemcpy(&s, w.q_size.p + fragment, 4, hipMemcpyDeviceToHost));
    *sketch_size = s;
    int c = std::min(s, cap);
    if (c > 0) FA_HIP(hipMemcpy(hashes, w.q_hash.p + (size_t)fragment * m->qcap, (size_t)c * 4, hipMemcpyDeviceToHost));
  });
}
int fa_debug_sketch_sequence(const fa_params *params, const void *data, int64_t length, int char_width, uint32_t *hash,
                             int32_t *wpos, int64_t cap, int64_t *n) {
  return guarded([&] {
    validate_params(*params);
    fa_sketch s;
    s.P = *params;
    s.reset_data();
    if (length >= params->kmer_size) {
      s.pending.append(data, char_width, length);
      s.book.pending_contig.push_back(0);
    }
    s.flush();
    *n = s.nrec;
    size_t c = (size_t)std::min<int64_t>(s.nrec, cap);
    if (c) {
      s.rec.hash.download(hash, c, s.stream);
      s.rec.wpos.download(wpos, c, s.stream);
      FA_HIP(hipStreamSynchronize(s.stream));
    }
    if (s.stream) (void)hipStreamDestroy(s.stream);
    if (s.up_stream) (void)hipStreamDestroy(s.up_stream);
  });
}

// development probe: how many 128-thread workgroups with `lds_bytes` of dynamic LDS does the chip hold at once, right now?
__global__ void k_probe_occupancy(unsigned *alive, unsigned *peak, int spin) {
  extern __shared__ unsigned char probe_lds[];
  if (threadIdx.x == 0) { unsigned a = atomicAdd(alive, 1u) + 1u; atomicMax(peak, a); }
  probe_lds[threadIdx.x] = (unsigned char)threadIdx.x;
  __syncthreads();
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  while (__builtin_amdgcn_s_memtime() - t0 < (unsigned long long)spin) __builtin_amdgcn_s_sleep(8);
  __syncthreads();
  if (threadIdx.x == 0) atomicSub(alive, 1u);
  if (probe_lds[(threadIdx.x + 1) & 63] == 255 && spin < 0) alive[1] = 1;
}
int fa_debug_probe_occupancy(int lds_bytes, int *peak_alive) {
  return guarded([&] {
    require_device();
    DevBuf<unsigned> d;
    d.ensure(16);
    FA_HIP(hipMemset(d.p, 0, 64));
    hipLaunchKernelGGL(k_probe_occupancy, dim3(4096), dim3(128), (size_t)lds_bytes, 0, d.p, d.p + 4, 200000);
    FA_HIP(hipDeviceSynchronize());
    unsigned h[8];
    FA_HIP(hipMemcpy(h, d.p, 32, hipMemcpyDeviceToHost));
    *peak_alive = (int)h[4];
  });
}
int fa_mapper_debug_items(fa_mapper *m, void *out, int64_t bytes) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    Workspace &w = m->ws[m->last_ws];
    FA_REQUIRE(bytes >= 0 && (size_t)bytes <= w.items.cap, FA_ERR_INVALID, "more bytes than the event arena holds");
    FA_HIP(hipMemcpy(out, w.items.p, (size_t)bytes, hipMemcpyDeviceToHost));
  });
}
int fa_mapper_debug_links(fa_mapper *m, int32_t *prev, int32_t *fwd, int32_t *bwd, uint8_t *flags, int64_t cap, int64_t *n) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    const size_t c = (size_t)std::max<int64_t>(0, std::min<int64_t>(m->N, cap));
    if (c) {
      FA_HIP(hipMemcpy(prev, m->rec_prev.p, c * 4, hipMemcpyDeviceToHost));
      FA_HIP(hipMemcpy(fwd, m->rec_fwd.p, c * 4, hipMemcpyDeviceToHost));
      FA_HIP(hipMemcpy(bwd, m->rec_bwd.p, c * 4, hipMemcpyDeviceToHost));
      FA_HIP(hipMemcpy(flags, m->rec_flags.p, c, hipMemcpyDeviceToHost));
    }
    *n = m->N;
  });
}
int fa_mapper_debug_locus_events(fa_mapper *m, uint32_t *events, int64_t cap, int64_t *n) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    Workspace &w = m->ws[m->last_ws];
    int64_t k = 0;
    if (holds_last_pass(w)) {
      for_each_locus_slice(w, [&](size_t first, size_t count) {
        const size_t c = (size_t)std::max<int64_t>(0, std::min<int64_t>((int64_t)count, cap - k));
        if (c) FA_HIP(hipMemcpyAsync(events + k, w.l_nev.p + first, c * 4, hipMemcpyDeviceToHost, w.stream));
        k += (int64_t)count;
      });
      FA_HIP(hipStreamSynchronize(w.stream));
    }
    *n = k;
  });
}
int fa_mapper_set_stage_events(fa_mapper *m, int on) {
  std::lock_guard<std::mutex> lock(m->mtx);
  m->stage_events = on != 0;
  return FA_OK;
}
int fa_mapper_last_timings(fa_mapper *m, float *ms, int n) {
  std::lock_guard<std::mutex> lock(m->mtx);
  for (int i = 0; i < n && i < MS_SLOTS; i++) ms[i] = m->ws[m->last_ws].last_ms[i];
  return FA_OK;
}
int fa_mapper_debug_spec(fa_mapper *m, int64_t *out, int n) {
  std::lock_guard<std::mutex> lock(m->mtx);
  const Spec &s = m->spec;
  const Forms &f = m->ws[m->last_ws].last_forms;
  auto ppm = [](float share) { return (int64_t)std::lround((double)share * 1e6); };
  const int64_t v[] = {s.init, s.smax, s.seed_slots, ppm(s.l1_small_share), ppm(s.l1_mid_share), ppm(s.l1_tiny_share),
                       s.l1_prefilter, s.l1_no_small, s.l2_loci_last, s.redo, s.part_frags, s.fuse_skip, s.fuse_penalty,
                       s.smax_misses, (int64_t)s.scratch_words, (int64_t)s.items_cap, s.l_cap,
                       f.n_l1, f.l1_threads[0], f.l1_threads[1], f.l1_threads[2], f.prefilter, f.scan_sorted, f.wide, f.fused,
                       f.ordered, f.redo, f.smax, f.seed_slots};
  for (int i = 0; i < n; i++) out[i] = i < (int)(sizeof(v) / sizeof(v[0])) ? v[i] : 0;
  return FA_OK;
}
int fa_mapper_stream(fa_mapper *m, void **stream) { *stream = (void *)m->stream; return FA_OK; }

int fa_bench_sketch_kernel(fa_mapper *m, fa_genomes *g, int repeat, float *ms_per_launch, uint64_t *bases, uint64_t *minimizers) {
  return guarded([&] {
    WorkspaceLease lease(*m);
    Workspace &w = *lease.w;
    require_device();
    int ntiles = (int)g->ntiles;
    FA_REQUIRE(ntiles > 0 && repeat > 0, FA_ERR_INVALID, "nothing to sketch");
    // the genome as REFERENCE sketching sees it: the fragments of a contig lie back to back in the batch's store, so they are
    // joined into whole sequences again and cut into the tiles reference sketching uses (k1_tile_len: positions + halo = whole
    // hashing trips); the batch's own tiles are per query fragment, for k_query_fused.  Batches with exceptions keep their tiles.
    const Tile *tiles = g->tiles;
    DevBuf<Tile> retiled;
    const int tile_len = k1_tile_len(m->P.window_size);
    if (g->store.n_exc == 0 && m->P.alphabet_size == 4) {
      std::vector<Tile> host((size_t)ntiles), cut;
      FA_HIP(hipMemcpy(host.data(), g->tiles, (size_t)ntiles * sizeof(Tile), hipMemcpyDeviceToHost));
      int64_t run_base = -1, run_len = 0;
      int32_t run_id = 0, last_seq = -1;
      auto close = [&] {
        if (run_base < 0) return;
        const int64_t npos = run_len - m->P.kmer_size + 1;
        for (int64_t p0 = 0; p0 < npos; p0 += tile_len)
          cut.push_back(Tile{run_base, (int32_t)run_len, (int32_t)p0, (int32_t)std::min<int64_t>(tile_len, npos - p0), run_id, 0, 0});
        run_id++; run_base = -1; run_len = 0;
      };
      // (a run ends where a contig ends, not only where the addresses break: a contig whose whole fragments fill a multiple of
      // 64 bases is followed by the next one without a gap, and k-mers / windows across that seam are not what reference
      // sketching hashes)
      size_t next_contig = 0;
      for (const Tile &t : host) {
        if (t.seq == last_seq) continue;                               // (the other tiles of a fragment seen already)
        last_seq = t.seq;
        bool starts_contig = false;
        while (next_contig < g->contig_frag_lo.size() && g->contig_frag_lo[next_contig] <= (int64_t)t.seq) { starts_contig = g->contig_frag_lo[next_contig] == (int64_t)t.seq; next_contig++; }
        if (!starts_contig && run_base >= 0 && t.base == run_base + run_len && run_len + t.seq_len < (1LL << 31)) run_len += t.seq_len;
        else { close(); run_base = t.base; run_len = t.seq_len; }
      }
      close();
      retiled.upload(cut, w.stream);
      tiles = retiled.p; ntiles = (int)cut.size();
    }
    w.last_ms[MS_TILE_LEN] = (float)tile_len;
    w.sk.stage_hash.ensure((size_t)ntiles * TILE);
    w.sk.stage_wpos.ensure((size_t)ntiles * TILE);
    w.sk.tile_count.ensure((size_t)ntiles + 1);
    hipEvent_t e0, e1;
    FA_HIP(hipEventCreate(&e0)); FA_HIP(hipEventCreate(&e1));
    launch_sketch_tiles(m->P, g->store, tiles, ntiles, w.sk.stage_hash.p, w.sk.stage_wpos.p, w.sk.tile_count.p, w.stream);
    FA_HIP(hipEventRecord(e0, w.stream));
    for (int i = 0; i < repeat; i++)
      launch_sketch_tiles(m->P, g->store, tiles, ntiles, w.sk.stage_hash.p, w.sk.stage_wpos.p, w.sk.tile_count.p, w.stream);
    FA_HIP(hipEventRecord(e1, w.stream));
    FA_HIP(hipEventSynchronize(e1));
    float ms = 0;
    FA_HIP(hipEventElapsedTime(&ms, e0, e1));
    *ms_per_launch = ms / repeat;
    std::vector<int32_t> counts((size_t)ntiles);
    w.sk.tile_count.download(counts.data(), (size_t)ntiles, w.stream);
    FA_HIP(hipStreamSynchronize(w.stream));
    uint64_t tot = 0;
    for (int c : counts) tot += (uint64_t)c;
    *minimizers = tot;
    *bases = g->total_bases;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  });
}

}  // extern "C"
