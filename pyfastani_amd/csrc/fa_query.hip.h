// fa_query.hip.h -- the query pipeline over a fragment range of a resident batch: one pass on one workspace (QueryPass),
// the call around the passes (run_query), the lease of a workspace, and what reads a finished pass back (the stage getters).
// Host side of the one translation unit fa_engine.hip.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <deque>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "fa_batch.hip.h"
#include "fa_common.h"
#include "fa_index.hip.h"
#include "fa_lease.h"
#include "fa_mapstream.h"
#include "fa_policy.h"

using namespace fa;

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
      const std::vector<int32_t> own = m.stats.pass_shared_at(w.rules.l2_confidence);
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
    uint32_t order_run = 0;                   // ... or, inside one genome, the run length of the arithmetic order (0: off)
    // into the status block of the part (launch_part, once the block exists)
    int32_t *d_stats = nullptr;
    uint64_t *d_totals = nullptr;
    uint32_t *d_counters = nullptr;
    unsigned long long *d_pinfo = nullptr;
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
    w.sk.reserve((size_t)std::max(ntiles, 1));
    w.q_hash.ensure((size_t)F * qcap); w.q_off.ensure((size_t)F * qcap); w.q_cnt.ensure((size_t)F * qcap);
    w.q_size.ensure((size_t)F); w.n_seeds.ensure((size_t)F); w.ovf_off.ensure((size_t)F);
    w.f_loci_lo.ensure((size_t)F); w.f_loci_n.ensure((size_t)F);
    w.status.ensure(1);
    if (!w.h_status) {
      w.pin_status.ensure(sizeof(PassStatus), hipHostMallocMapped | hipHostMallocCoherent);
      w.h_status = (PassStatus *)w.pin_status.p;
      memset(w.h_status, 0, sizeof(PassStatus));
    }
    p.d_stats = w.status.p->stats; p.d_totals = w.status.p->totals; p.d_counters = w.status.p->counters; p.d_pinfo = w.status.p->pinfo;
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

  // The workgroup order of k_l2_events (frag_order_gate).  A part inside ONE genome -- a caller that maps genome after genome
  // out of a resident batch changes the range with every call -- takes it as arithmetic on the workgroup number (one_genome_run,
  // one_genome_frag): nothing is built, cached or uploaded.  A part of several genomes takes a table (build_frag_order), built
  // on the host, cached per (batch, fragment range) and uploaded behind K1.
  void prepare_order(Part &p) {
    // (FA_FRAG_ORDER_ONE: the A/B of the one-genome order)
    if (!frag_order_gate(knob::frag_order() != 0, knob::frag_order_one() != 0, NQ, p.F)) return;
    if (frag_range_in_one_genome(g.genome_frag_lo.data(), g0, p.f0, p.f1)) { p.order_run = one_genome_run(p.F); return; }
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
    const uint32_t seed_slots = p.l1.seed_slots();
    // ---- seed totals and speculation checks (the lookup itself is the tail of k_query_sketch).  A kernel of its own
    //      only where k_l1 / k_l1_big need the scratch offsets it produces; else workgroup F of k_l1's launch ----
    const bool fold_totals = sp.scratch_words == 0;
    if (!fold_totals)
      hipLaunchKernelGGL(k_seed_totals, dim3(1), dim3(1024), 0, st, w.n_seeds.p, F, seed_slots, p.d_totals, w.ovf_off.p,
                         p.d_stats, smax, sp.scratch_words, p.d_pinfo, &w.status.p->stamp[1], w.q_size.p);
    debug_sync(st, "lookup");
    // ---- L1 ----
    {
      L1Args a;
      a.fold_totals = fold_totals ? 1 : 0; a.spec_smax = smax; a.F = F; a.totals = p.d_totals; a.stats = p.d_stats;
      a.spec_scratch_words = sp.scratch_words; a.stamp = &w.status.p->stamp[1];
      a.ix = ix; a.q_size = w.q_size.p; a.q_off = w.q_off.p; a.q_cnt = w.q_cnt.p; a.n_seeds = w.n_seeds.p;
      a.ovf_off = w.ovf_off.p; a.ovf_buf = w.ovf_buf.p; a.min_hits_lut = w.lut_min_hits;
      a.l_frag = w.l_frag.p; a.l_seq = w.l_seq.p; a.l_start = w.l_start.p; a.l_end = w.l_end.p; a.l_group = w.l_group.p;
      a.l_rfirst = w.l_rfirst.p; a.l_rlast = w.l_rlast.p; a.l_rpart = w.l_rpart.p;
      a.counters = p.d_counters; a.loci = p.loci; a.qcap = qcap; a.frag_len = m.P.fragment_length; a.l_cap = (int32_t)l_cap;
      a.lds_seed_cap = seed_slots; a.totals_seed_cap = seed_slots; a.n_lo = 0; a.n_hi = 0xFFFFFFFFu; a.pinfo = p.d_pinfo; a.lut_smax = smax; a.scratch_words = sp.scratch_words;
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
    const bool wide = p.wide;
    // ---- L2: event streams, then the sequential slide (uint8 state, uint16 redo) ----
    {
      if (m.stage_events) FA_HIP(hipEventRecord(w.ev[0], st));
      L2Args a;
      a.stamp = &w.status.p->stamp[2];
      a.ix = ix; a.q_hash = w.q_hash.p; a.q_size = w.q_size.p;
      a.l_frag = w.l_frag.p; a.l_seq = w.l_seq.p; a.l_start = w.l_start.p; a.l_end = w.l_end.p; a.l_group = w.l_group.p;
      a.l_rfirst = w.l_rfirst.p; a.l_rlast = w.l_rlast.p; a.l_rpart = w.l_rpart.p; a.frag_len = m.P.fragment_length;
      a.l_beg = w.l_beg.p; a.l_end0 = w.l_end0.p; a.l_last = w.l_last.p; a.l_nev = w.l_nev.p; a.l_ioff = w.l_ioff.p; a.l_ndrop = w.l_ndrop.p;
      a.items = w.items.p; a.items_cap = sp.items_cap; a.pinfo = p.d_pinfo; a.l_cap = (int32_t)l_cap;
      a.l_shared = w.l_shared.p; a.l_pos = w.l_pos.p; a.pass_lut = w.lut_pass; a.group_best = w.group_best.p;
      a.counters = p.d_counters; a.loci = p.loci; a.qcap = qcap; a.cmw = m.cmw;
      a.cnt_slots = smax + 1;
      a.rec_total = (unsigned long long *)&p.d_totals[TOT_RECORDS];
      a.ev_region = w.status.p->ev_region; a.rec_region = w.status.p->rec_region;
      a.n_regions = ev_regions_for(F);
      a.region_cap = (sp.items_cap / a.n_regions) & ~7ULL;
      a.l_redo = w.l_redo.p;
      a.redo_count = &p.d_counters[CNT_WIDE];
      const L2Lds lds(m.P, smax, wide);
      a.scan_class_div = p.scan_sorted ? lds.scan_class_div : 0;
      a.scan_hist = w.scan_hist.p; a.scan_cursor = w.scan_hist.p + LOCI_REGIONS * SCAN_CLASSES;
      a.scan_order = p.scan_sorted ? w.scan_order.p : nullptr;
      a.slide_end = w.rules.slide_end; a.tie = TieKey::of(w.rules.cgi_ties);
      a.f_loci_lo = w.f_loci_lo.p; a.f_loci_n = w.f_loci_n.p;
      // several genomes in the pass: the workgroups of k_l2_events in offset-major order (prepare_order)
      // (one genome: the same order as arithmetic, 8 runs of order_run workgroups)
      a.frag_order = p.frag_order;
      a.one_run = p.order_run; a.one_frags = (uint32_t)F;
      const uint32_t ev_grid = p.order_run ? 8u * p.order_run : p.frag_order ? p.order_len : (uint32_t)F;
      if (p.frag_order || p.order_run) r.ordered = true;
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
    if (m.stage_events) FA_HIP(hipEventRecord(w.ev[1], st));
  }

  // core-genome identity and the one hand-over of the part
  void launch_cgi_stage_and_hand_over(Run &r, Part &p) {
    const Spec &sp = p.sp;
    const int64_t f0 = p.f0;
    const int64_t l_cap = p.l_cap;
    // ---- core-genome identity ----
    if (npairs > 0) {
      CgiArgs a;
      a.stamp = &w.status.p->stamp[3];
      a.ix = ix; a.group_best = w.group_best.p; a.counters = p.d_counters; a.l_frag = w.l_frag.p; a.l_seq = w.l_seq.p;
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
      FA_HIP(hipEventSynchronize(w.ev[1]));
      FA_HIP(hipEventElapsedTime(&ev_ms, w.ev[0], w.ev[1]));
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
    for (Event &e : w.ev) e.get();
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
          try { w.stream.get(); } catch (const Error &) { throw Error(FA_ERR_NO_DEVICE, "hipStreamCreate failed"); }
        }) {}
};

// the one-query-at-a-time call (fa_mapper_query and its siblings): upload into the workspace's recycled batch, then run_query
static void query_one_call(fa_mapper *m, const void *const *contigs, const int64_t *lengths, int n_contigs, int char_width,
                           fa_cgi_row *rows, int64_t cap, int64_t *n_rows, int *n_short, uint64_t *total_fragments,
                           uint64_t *total_length, const MapRequest *want) {
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
}

// the live loci of a part, region by region (LociRegions): fn(first locus number, count)
template <class Fn>
static void for_each_locus_slice(const Workspace &x, Fn fn) {
  for (uint32_t r = 0; r < x.loci_n && r < (uint32_t)LOCI_REGIONS; r++)
    if (x.last_region_count[r]) fn((size_t)r << x.loci_shift, (size_t)x.last_region_count[r]);
}

// The workspace holds the intermediates of the last part it ran.  A pass that ran in more parts (several passes of one
// genome, or parts that were repeated) has left only its last part behind: say so instead of handing out a fraction of
// the pass as if it were all of it.  Returns whether the workspace holds a pass at all.
static bool holds_last_pass(const Workspace &w) {
  FA_REQUIRE(w.last_F == w.pass_F, FA_ERR_UNSUPPORTED,
             "the stage getters hold the last part of every lane only, and the last pass ran in more parts than that");
  return w.last_F > 0;
}

// What every stage getter opens with: the mapper's lock, its device, the workspace of the most recent call and whether that
// holds a pass (holds_last_pass).  copy() takes the live loci of that pass, slice by slice, from each source array (32-bit
// words on the device) to its destination on the host, clipped to `cap` loci, synchronises, and returns the number of loci.
struct LastPass {
  struct Column { void *dst; const void *src; };
  std::lock_guard<std::mutex> lock;
  Workspace &w;
  const bool held;
  explicit LastPass(fa_mapper *m) : lock(m->mtx), w((bind_device(m->device), m->ws[m->last_ws])), held(holds_last_pass(w)) {}
  int64_t copy(std::initializer_list<Column> columns, int64_t cap) const {
    int64_t k = 0;
    if (!held) return k;
    for_each_locus_slice(w, [&](size_t first, size_t count) {
      const size_t c = (size_t)std::max<int64_t>(0, std::min<int64_t>((int64_t)count, cap - k));
      if (c) for (const Column &col : columns)
        FA_HIP(hipMemcpyAsync((uint32_t *)col.dst + k, (const uint32_t *)col.src + first, c * 4, hipMemcpyDeviceToHost, w.stream));
      k += (int64_t)count;
    });
    FA_HIP(hipStreamSynchronize(w.stream));
    return k;
  }
};

// fa_bench_sketch_kernel: K1 alone over a resident batch, as reference sketching would launch it
static void bench_sketch_kernel(fa_mapper *m, fa_genomes *g, int repeat, float *ms_per_launch, uint64_t *bases, uint64_t *minimizers) {
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
  w.sk.reserve((size_t)ntiles);
  Event e0, e1;
  e0.get(); e1.get();
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
}
