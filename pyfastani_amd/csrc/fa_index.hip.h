// fa_index.hip.h -- fa_mapper: the indexed reference (build_index: Sketch_t::index + computeFreqHist on the device), its
// lookup tables, and the workspaces its query calls borrow (Workspace, MapStage).  The pass that runs on a workspace is
// fa_query.hip.h.  Host side of the one translation unit fa_engine.hip; fa_mapper is the C ABI's opaque type, hence the
// global namespace.
#pragma once

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <climits>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <vector>

#include "fa_common.h"
#include "fa_diag.h"
#include "fa_k1.hip.h"
#include "fa_knobs.h"
#include "fa_map.hip.h"
#include "fa_policy.h"
#include "fa_stats.h"

using namespace fa;

struct fa_genomes;   // (fa_batch.hip.h: a workspace keeps the batch of the one-query call, by pointer)

// (the slots of Workspace::last_ms, TimingSlot, come from the table of fa_diag.h)

// The way of the mapping records to the host: two buffers of `records` fa_hit_mapping in HBM, two in pinned host memory and an
// event each.  k_map_write fills HBM buffer w & 1 with window w of a pass (fa_mapstream.h), an asynchronous copy takes it to
// pinned buffer w & 1, and while the host consumes that the device works on window w + 1.  Their size is the mapper's
// (fa_mapper_set_mapping_stage), not the table's; allocated by the first call that wants mappings on the host.
struct MapStage {
  fa_hit_mapping *dev[2] = {nullptr, nullptr}, *pin[2] = {nullptr, nullptr};
  Event ev[2];
  int64_t records = 0;
  MapStage() = default;
  MapStage(const MapStage &) = delete;
  MapStage &operator=(const MapStage &) = delete;
  ~MapStage() { release(); }
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
      ev[i].get(hipEventDisableTiming);
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
  // (members go in reverse order: the stream is destroyed before the pinned status block that its last kernel writes)
  PinnedBuf pin_status;               // mapped and coherent, written by k_publish_status
  PassStatus *h_status = nullptr;     // = pin_status.p once allocated
  Stream stream;
  SketchWork sk;
  DevBuf<uint32_t> q_hash, q_off, q_cnt, n_seeds, ovf_off, ovf_buf;
  DevBuf<PassStatus> status;
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
  Event ev[2];                        // around the L2 stage (fa_mapper_set_stage_events)
  int64_t pass_F = 0;                 // fragments of the last pass
  // the kernel forms of a part (fa_mapper_debug_spec): those of the part in flight, and those of the last part accepted in the
  // last call (cleared when a call starts)
  Forms forms, last_forms;
  // the one-query-at-a-time call (fa_mapper_query) recycles its batch object -- no device allocation per call -- and
  // builds the upload image in pinned memory; its rows come back through a pinned block too
  std::unique_ptr<fa_genomes> query_batch;
  PinnedBuf pin_image, pin_rows;
};

// ------------------------------------------------------------------------------------------------------------
// fa_mapper: the indexed reference + the workspace of the query pipeline
// ------------------------------------------------------------------------------------------------------------
struct fa_mapper {
  fa_params P;
  int device = -1;
  Stream stream;
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

// fa_stats.h: stat_zero_passes_alone.  Checked on every call (a mapper whose tables grew into such a sketch size stays refused).
static void require_no_zero_pass(const StatTables &t) {
  if (t.zero_pass)
    throw Error(FA_ERR_UNSUPPORTED, "percentage_identity " + std::to_string(t.pid) + " at l2_confidence " + std::to_string(t.ci) +
                " passes a mapping of no shared record, and none of one shared record, at sketch size " + std::to_string(t.zero_pass) +
                ", which the mapping tables cannot carry");
}

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
  require_no_zero_pass(m.stats);
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
