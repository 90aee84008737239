// fa_policy.h -- the policy of a query pass: plain C++, no HIP (scripts/host_sanitize/driver.cpp checks it on the CPU).
//
// A query pass runs in parts (fragment ranges).  Sizes that are only known on the device -- the largest sketch, the seed
// hits, the loci, the slide events -- are speculated from earlier parts (Spec), checked by the kernels, which raise SPEC_*
// flags in the status block (PassStatus), and judged here once the part is done: accepted, or void and run again with a
// grown record, or cut into smaller parts.  The same record picks the forms of the next part (the k_l1 size classes, the
// block pre-filter, the sorted scan, the wide state, the back-off of the fused sketch kernel).  fa_query.hip.h (QueryPass)
// owns the buffers, the launches and the locking; everything here is pure arithmetic over plain structs.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "fa_error.h"

#if defined(__HIPCC__)
#define FA_POLICY_FN __host__ __device__ inline
#else
#define FA_POLICY_FN inline
#endif

namespace fa {

// ------------------------------------------------------------------------------------------------------------
// constants shared with the kernels (fa_map.hip.h includes this header)
// ------------------------------------------------------------------------------------------------------------
// loci of one fragment merged in LDS by k_l1 (more fall back to a second pass that writes them to HBM).  128, not 256: with
// 3 KB of stage instead of 6 the kernel's 21.7 KB let seven workgroups share a CU, i.e. the 1666 fragments of a 5 Mb query run
// in ONE resident round (85 -> 81 us; 928 -> 872 us at 16 queries per launch); a fragment has one locus per related contig
constexpr int L1_STAGE = 128;
// the size classes of k_l1 (hits of a fragment): up to 16 per thread of the 256-thread form; up to the slots the 512-thread,
// 16-per-thread form is given (a kilobyte short of 16 x 512: see plan_l1); everything beyond
constexpr uint32_t L1_SMALL_HITS = 16u * 256u, L1_MID_HITS = 16u * 512u - 256u;
constexpr int L1_INPLACE_MAX = 32;  // most seeds per thread the in-place merge keeps in registers (template parameter E: 16 or 32)
// loci are numbered per region (LociRegions, fa_map.hip.h); slide events are reserved per region of the event arena
constexpr int LOCI_REGIONS = 64;
constexpr int EV_REGIONS = 64;
// rank bits of the 16-bit slide event (EvBits<uint16_t>): sketches up to 510 minimizers; larger ones take the wide events
constexpr int EV_RANK16 = 9;
// loci of one fragment whose descriptors (record range, drops, offset in the fragment's events) k_l2_events keeps in LDS between
// its head and its locus loop; the loci behind them are read back from the global arrays (the bench: about 55 per fragment)
constexpr int EV_LOCI_LDS = 64;

// Pass-level speculation.  A query pass is launched without intermediate host synchronisation, sized by what earlier
// passes needed (largest sketch, LDS seed slots, HBM seed scratch, loci and event capacities).  Kernels check those
// bounds on the device, skip the work that does not fit and raise a flag; the host reads the flags once at the end of
// the pass and, if any is set, grows the bounds and runs the pass again.
constexpr uint32_t SPEC_SMAX = 1, SPEC_SCRATCH = 2, SPEC_LOCI = 4, SPEC_EVENTS = 8, SPEC_QFUSE = 16;
constexpr uint32_t SPEC_LAST = SPEC_QFUSE;          // (the highest flag: a new one goes above it and moves this)
// The flags that void a part: all of them.  k_l2_order and k_l2_scan return early on ANY bit of pinfo[PI_FLAGS] (a void
// part made no order, and its scan would read one), which is only right because judge_part voids on every flag.  A flag
// that does not void would have to be kept out of those returns first.
constexpr uint32_t SPEC_VOID = SPEC_SMAX | SPEC_SCRATCH | SPEC_LOCI | SPEC_EVENTS | SPEC_QFUSE;
static_assert(SPEC_VOID == 2 * SPEC_LAST - 1, "every SPEC_* flag voids the part (k_l2_order / k_l2_scan rely on it)");

// ------------------------------------------------------------------------------------------------------------
// the status block of a pass
// ------------------------------------------------------------------------------------------------------------
// named slots of PassStatus::stats / totals / counters / pinfo (the kernels write them, judge_part and the accounting read them)
enum StatSlot : int {
  STAT_SMAX = 0,                // largest query sketch (seed_totals)
  STAT_SMALL, STAT_MID, STAT_TINY,   // fragments in the small / middle size class of k_l1, and up to half the small bound
};
enum TotalSlot : int {
  TOT_SEEDS = 0,                // seed hits of the part
  TOT_MAX_FRAG,                 // seed hits of the largest fragment
  TOT_SCRATCH,                  // HBM scratch words of the fragments that do not fit the LDS seed slots
  TOT_RECORDS,                  // reference records inside the locus ranges (fused L2 form)
};
enum CounterSlot : int {
  CNT_MERGED = 0,               // fragments k_l1 merged instead of block-sorting
  CNT_OFF_FAST,                 // fragments on the HBM road / cut by k_l1_big
  CNT_LOCI_OVF,                 // a loci region overflowed
  CNT_WIDE,                     // loci that need the wide L2 state
  CNT_ROWS_DONE,                // finished workgroups of k_cgi_rows
  CNT_L1_SORTED, CNT_L1_MERGED, // FA_L1_STATS samples: fragments block-sorted / merged by k_l1
};
enum PinfoSlot : int {
  PI_EVENTS = 0,                // slide events reserved (fused L2 form)
  PI_FLAGS,                     // SPEC_* flags
};

// Every small counter / statistic of a pass in ONE device block, mirrored into pinned host memory by one copy.
struct PassStatus {
  int32_t stats[4];                 // StatSlot
  int32_t total_rows, pad0;
  int64_t total_maps;               // fa_hit_mapping records of the pass (a call that asked for mappings; k_chunk_scan)
  uint64_t totals[4];               // TotalSlot
  uint32_t counters[8];             // CounterSlot
  unsigned long long pinfo[4];      // PinfoSlot
  unsigned long long ev_region[EV_REGIONS], rec_region[EV_REGIONS];   // k_l2_events: events reserved / records read per arena region
  uint32_t loci_region[LOCI_REGIONS];                                  // k_l1: loci reserved per region (LociRegions)
  unsigned long long dbg[16];       // FA_L1_STATS=1: shader-clock ticks of k_l1's phases, summed over the sampled workgroups (thread 0's view); [8..10] why block sorts gave up
  unsigned long long stamp[6];      // stage_stamp: pass start, lookup, L2, CGI, end (100 MHz ticks); not cleared with the rest
  uint32_t seq, pad1;               // host copy only: number of the pass whose status this is (k_publish_status)
};
static_assert(offsetof(PassStatus, stamp) % 16 == 0, "k_clear zeroes whole 16-byte words: the cleared prefix of the status block must end on one");

// ------------------------------------------------------------------------------------------------------------
// the speculation record
// ------------------------------------------------------------------------------------------------------------
// data-dependent sizes speculated from earlier passes; one per mapper, shared by all its workspaces (under its lock)
struct Spec {
  bool init = false;
  int smax = 0;
  uint32_t seed_slots = 0;
  uint64_t scratch_words = 0, items_cap = 0;
  int64_t l_cap = 0;
  int64_t part_frags = 0;   // fragments per part of a pass (shrinks when a part overflows the 32-bit workspace)
  bool redo = false;        // launch the wide-state scan as well (set once a locus overflowed the one-byte state)
  // k_query_fused met a fragment with more records than its LDS holds: the void range runs again through the two kernels
  // (`fuse_off`, a property of that attempt only).  The mapper keeps a back-off, not a verdict: the first overflow costs
  // nothing afterwards, consecutive ones skip 1, 3, 7 ... 63 passes before the fused form is tried again, and a fused pass
  // that is accepted clears the record -- one dense fragment no longer decides every later query of the mapper.
  bool fuse_off = false;
  int fuse_skip = 0, fuse_penalty = 0;
  int smax_misses = 0;      // times the largest sketch outgrew the bound (the first growth is tight, later ones are not)
  // share of the fragments of the last accepted part in the two lower size classes of k_l1 (-1: not seen yet)
  float l1_small_share = -1.0f, l1_mid_share = -1.0f, l1_tiny_share = -1.0f;   // (tiny: up to half the small class's bound)
  bool l1_prefilter = false;  // an accepted part saw fragments fall off k_l1's block sort: later passes drop dead hits before the sort (sticky)
  int64_t l2_loci_last = 0;   // loci of the last accepted part: k_l2_scan sorts its loci by stream length when there are waves to balance
  bool l1_no_small = false;   // ... and they still did with the pre-filter on and the 256-thread class in use: its table is too small for this index (sticky)
};

// the record at a mapper's first query (the engine reads the FA_* hooks that override these)
inline Spec spec_first_use(int smax, int64_t l_cap, uint64_t items_cap, int64_t part_frags) {
  Spec s;
  s.init = true;
  s.smax = smax;
  s.seed_slots = 4096;
  s.scratch_words = 0;
  s.l_cap = l_cap;
  s.items_cap = items_cap;
  s.part_frags = part_frags;
  return s;
}

// what a finished attempt learnt, into the mapper's record: bounds only grow, part_frags only shrinks, the LDS seed slots and
// the shares follow the latest pass, redo / l1_prefilter / l1_no_small are sticky (the fuse back-off is not merged: fuse_*)
inline void spec_merge(Spec &ms, const Spec &sp) {
  ms.smax = std::max(ms.smax, sp.smax);
  ms.seed_slots = sp.seed_slots;
  ms.scratch_words = std::max(ms.scratch_words, sp.scratch_words);
  ms.items_cap = std::max(ms.items_cap, sp.items_cap);
  ms.l_cap = std::max(ms.l_cap, sp.l_cap);
  ms.part_frags = std::min(ms.part_frags, sp.part_frags);
  ms.redo = ms.redo || sp.redo;
  ms.l1_small_share = sp.l1_small_share; ms.l1_mid_share = sp.l1_mid_share; ms.l1_tiny_share = sp.l1_tiny_share;
  ms.l1_prefilter = ms.l1_prefilter || sp.l1_prefilter; ms.l1_no_small = ms.l1_no_small || sp.l1_no_small;
  ms.l2_loci_last = sp.l2_loci_last;
  ms.smax_misses = std::max(ms.smax_misses, sp.smax_misses);
}

// the back-off of k_query_fused (Spec::fuse_*), applied to the mapper's record
inline void fuse_overflowed(Spec &ms) {                        // a part overflowed the fused kernel's LDS
  ms.fuse_penalty = ms.fuse_penalty ? std::min(64, ms.fuse_penalty * 2) : 1;
  ms.fuse_skip = ms.fuse_penalty - 1;
}
// an accepted part: a fused one clears the back-off; one that skipped the fused form serves a pass of it (`skipped`: the
// attempt started with fuse_off and was not the forced repeat of an overflow)
inline void fuse_accepted(Spec &ms, bool fused, bool skipped) {
  if (fused) ms.fuse_penalty = 0;
  else if (skipped && ms.fuse_skip > 0) ms.fuse_skip--;
}

// ------------------------------------------------------------------------------------------------------------
// pure helpers
// ------------------------------------------------------------------------------------------------------------
inline int floor_log2(int v) {
  int l = 0;
  while (((int64_t)2 << l) <= v) l++;                          // (64-bit: 2 << 30 would overflow an int for v >= 2^30)
  return l;
}

// regions of the event arena used by a part of F fragments (L2Args::n_regions): a power of two, one per sixteen fragments
inline uint32_t ev_regions_for(int64_t F) {
  uint32_t n = 1;
  while (n < (uint32_t)EV_REGIONS && (int64_t)n * 16 <= F) n <<= 1;
  return n;
}

// seed hits of one fragment sorted in LDS by k_l1 (4 bytes each); more go through HBM scratch
inline uint32_t lds_seed_cap_max(int smax) {
  // (the dynamic request of k_l1 -- l1_lds_bytes: seeds, list offsets and sources, six staged locus arrays -- plus its static
  // LDS, a few hundred bytes, must stay within the 160 KB of a CU)
  const int64_t room = 160 * 1024 - 2048 - (int64_t)L1_STAGE * 6 * 4 - std::max<int64_t>(((int64_t)smax + 2) * 8, 1024 * 10) - 64;
  return (uint32_t)std::max<int64_t>(256, room / 4 / 256 * 256);
}

// A tri-state knob (-1: unset): the policy's default, or forced off (0) / on (anything else).
inline bool knob_or(int knob, bool dflt) { return knob < 0 ? dflt : knob != 0; }

// Workgroup order of k_l2_events over the F fragments of a pass that lie in ONE genome (round 5): its fragments in eight
// contiguous runs of `run` = ceil(F / 8), one per XCD (workgroups go to XCDs round robin, so workgroup b runs on XCD b mod 8 and is
// the (b / 8)-th of it).  The loci of neighbouring fragments overlap by two thirds on every reference (a locus spans ~2.6 fragment
// lengths), so the workgroups of a run read the same index stretches -- from their XCD's L2 instead of the memory side, where
// the identity order (fragment b on XCD b mod 8) had put every neighbour on another XCD.  8 x run workgroups; the fragment
// (relative to the pass) of workgroup b, or -1: the last run may be short.  Under 64 fragments the identity order stays (run 0).
FA_POLICY_FN uint32_t one_genome_run(int64_t F) { return F < 64 ? 0u : (uint32_t)((F + 7) / 8); }
FA_POLICY_FN int32_t one_genome_frag(uint32_t b, uint32_t run, uint32_t F) {
  const uint32_t i = (b & 7u) * run + (b >> 3);
  return (b >> 3) < run && i < F ? (int32_t)i : -1;
}
FA_POLICY_FN int32_t one_genome_frag(uint32_t b, uint32_t F) { return one_genome_frag(b, (F + 7u) / 8u, F); }
// do the fragments [f0, f1) lie in one genome?  (genome_frag_lo: the first fragment of every genome of the batch, g0 one at or
// before f0)
inline bool frag_range_in_one_genome(const int64_t *genome_frag_lo, int32_t g0, int64_t f0, int64_t f1) {
  int32_t q = g0;
  while (genome_frag_lo[q + 1] <= f0) q++;
  return genome_frag_lo[q + 1] >= f1;
}

// Workgroup order of k_l2_events over the fragments [f0, f1) of a pass that holds several genomes (genome_frag_lo: the
// first fragment of every genome of the batch, g0 the first genome of the pass): fragments sorted by their offset inside
// their genome (then by genome), every group of equal offset dealt to the XCD whose list is the shortest so far
// (equal-sized genomes: group p lands on XCD p mod 8), and the eight lists interleaved the way workgroups are dispatched
// (workgroup b runs on XCD b mod 8); -1 pads the shorter lists.  Returns 0 -- the caller keeps the identity order -- when
// the lists cannot be balanced: fewer groups than XCDs (a batch of plasmids or viral contigs of one or two fragments each
// would put every real workgroup on one XCD) or more than 15 % of padding.
inline uint32_t build_frag_order(const int64_t *genome_frag_lo, int32_t g0, int64_t f0, int64_t f1, std::vector<int32_t> &out) {
  const int64_t F = f1 - f0;
  out.clear();
  int32_t q = g0;
  while (genome_frag_lo[q + 1] <= f0) q++;
  if (frag_range_in_one_genome(genome_frag_lo, g0, f0, f1)) {
    // ONE genome: the order is arithmetic (one_genome_frag), and a pass takes it from there without a table (QueryPass::
    // prepare_order); this is the same order as a table, for the callers and the checks that want one
    const uint32_t run = one_genome_run(F);
    if (!run) return 0;
    out.resize((size_t)run * 8);
    for (uint32_t b = 0; b < run * 8; b++) out[b] = one_genome_frag(b, run, (uint32_t)F);
    return (uint32_t)out.size();
  }
  // offset of every fragment inside its genome, counting sort by it (stable: genomes stay in order inside a group)
  std::vector<int32_t> off((size_t)F);
  int32_t max_off = 0;
  for (int64_t i = 0, qq = q; i < F; i++) {
    while (genome_frag_lo[qq + 1] <= f0 + i) qq++;
    off[(size_t)i] = (int32_t)(f0 + i - genome_frag_lo[qq]);
    max_off = std::max(max_off, off[(size_t)i]);
  }
  if (max_off + 1 < 8) return 0;
  std::vector<int32_t> start((size_t)max_off + 2, 0);
  for (int64_t i = 0; i < F; i++) start[(size_t)off[(size_t)i] + 1]++;
  for (int32_t p = 0; p <= max_off; p++) start[(size_t)p + 1] += start[(size_t)p];
  std::vector<int32_t> sorted((size_t)F), fill(start.begin(), start.end() - 1);
  for (int64_t i = 0; i < F; i++) sorted[(size_t)fill[(size_t)off[(size_t)i]]++] = (int32_t)i;
  // groups -> XCD lists (the shortest list takes the next group; ties to the lowest XCD), then interleave
  size_t len[8] = {0};
  std::vector<uint8_t> xcd_of((size_t)max_off + 1);
  for (int32_t p = 0; p <= max_off; p++) {
    int x = 0;
    for (int i = 1; i < 8; i++) if (len[i] < len[x]) x = i;
    xcd_of[(size_t)p] = (uint8_t)x;
    len[x] += (size_t)(start[(size_t)p + 1] - start[(size_t)p]);
  }
  const size_t longest = *std::max_element(len, len + 8);
  if ((double)longest * 8.0 > 1.15 * (double)F) return 0;
  out.assign(longest * 8, -1);
  size_t at[8] = {0};
  for (int32_t p = 0; p <= max_off; p++) {
    const size_t x = xcd_of[(size_t)p];
    for (int32_t i = start[(size_t)p]; i < start[(size_t)p + 1]; i++) out[(at[x]++) * 8 + x] = sorted[(size_t)i];
  }
  return (uint32_t)out.size();
}

// ------------------------------------------------------------------------------------------------------------
// the forms of a part
// ------------------------------------------------------------------------------------------------------------
// the kernel forms of a part (fa_mapper_debug_spec; judge_part reads those the part ran with)
struct Forms {
  int n_l1 = 0, l1_threads[3] = {0, 0, 0};
  bool prefilter = false, scan_sorted = false, wide = false, fused = false, ordered = false, redo = false;
  int smax = 0;
  uint32_t seed_slots = 0;
  bool small_class() const { return n_l1 > 1 && l1_threads[0] == 256; }   // the 256-thread class ran next to another class
};

// one launch of k_l1: the fragments with n_lo <= hits <= n_hi, `slots` LDS seed slots, `nt` threads
struct L1Class { int nt; uint32_t slots, n_lo, n_hi; };
struct L1Plan {
  L1Class c[3];
  int n = 0;
  bool prefilter = false;       // the part drops dead hits before k_l1's block sort
  uint32_t need = 0;            // the speculated slots, within what LDS holds
  uint32_t seed_slots() const { return c[n - 1].slots; }   // "fits LDS" for seed_totals and k_l1_big: the last class's slots
};
// the FA_* overrides of plan_l1 (FA_L1_PREFILTER: -1 unset; FA_L1_THIN_SMALL: < 0 unset; FA_L1_THIN_MID)
struct L1Knobs { int prefilter = -1; float thin_small = -1.0f, thin_mid = 0.05f; };

// The k_l1 launches of a part over an index of `records` records.
// LDS also holds smax list offsets; the in-place merge keeps at most 32 seeds per thread in registers
// k_l1 runs once per size class of fragments (L1Args::n_lo / n_hi): up to 4 096 hits the 256-thread form with 16 hits per
// thread (4-wave workgroups, eight per CU: a 5 Mb query is one round of workgroups), up to 7 936 the 512-thread form with 16,
// beyond the 512-thread form with 32 (above 4 096 hits 512 threads measured best: fewer hits per thread shorten every thread's
// chain of dependent LDS round trips; 1 024 threads pay more for barriers than they gain).  A class the speculated bound
// (sp.seed_slots: the largest fragment seen, plus a quarter) does not reach is not launched; the last class takes everything
// above its lower bound, overflow into HBM scratch included.
inline L1Plan plan_l1(const Spec &sp, int64_t records, const L1Knobs &k) {
  L1Plan p;
  const uint32_t cap_max = lds_seed_cap_max(sp.smax), need = std::min(sp.seed_slots, cap_max);
  p.need = need;
  const uint32_t s_slots = std::min<uint32_t>(need, L1_SMALL_HITS);
  p.c[p.n++] = L1Class{256, s_slots, 0u, need <= L1_SMALL_HITS ? 0xFFFFFFFFu : s_slots};
  if (need > L1_SMALL_HITS) {
    // (a 512-thread workgroup is eight waves: four of them fill a CU whatever their LDS up to 39 KB, so the block table of
    // l1_block_sort -- a third as many entries as seed slots -- gets all the slots the 16-per-thread form can address)
    // (7 936, not 8 192: the kilobyte goes to the key buffer behind the slots, which then holds the (key, place) pairs of 1 024
    // blocks -- the 4 x 10^8-record index of config 3 adds ~500 chance hits, each a block of its own, to the ~250 blocks of a
    // fragment's relatives -- and four workgroups still fill a CU)
    const uint32_t m_slots = std::min<uint32_t>(L1_MID_HITS, cap_max);
    p.c[p.n++] = L1Class{512, m_slots, s_slots + 1u, need <= m_slots ? 0xFFFFFFFFu : m_slots};
    if (need > m_slots)
      p.c[p.n++] = L1Class{512, std::min<uint32_t>(need, (uint32_t)(L1_INPLACE_MAX * 512)), m_slots + 1u, 0xFFFFFFFFu};
  }
  // The pre-filter of the block sort (l1_block_sort: hits that cannot belong to a candidate are dropped before the sort, one more
  // sweep over the position lists) pays where chance hits push the blocks of a fragment beyond what the register sort holds, and
  // costs where they do not (profiles/r06_l1_prefilter.txt: lookup + L1 70.4 -> 60.9 ms on config 3, 211 -> 156 on 2000 x 2000
  // genomes, 38.9 -> 20.1 in the (k = 14, fragment 1000) cell, whose 28-bit hashes collide everywhere; 52.8 -> 66.3 us on the
  // one-query step, 5.4 -> 6.2 ms in the (16, 3000) cell).  So it follows the evidence: on from 3 x 10^8 index records (~400
  // chance hits per fragment), and on any index once an accepted part of this mapper had one fragment in two hundred fall back
  // to the merge (Spec::l1_prefilter, sticky).  FA_L1_PREFILTER = 0 / 1: never / always.
  p.prefilter = knob_or(k.prefilter, records >= 300000000LL || sp.l1_prefilter);
  // Which classes get a launch of their own is decided from the shares `seed_totals` counted in the last accepted part (a launch
  // walks every fragment: 1.7 million workgroups that return at once cost config 3 two milliseconds of 67).  Measured (round 6,
  // profiles/r06_l1_classes_ab.txt, r06_l1_prefilter.txt): fragments of ~1 500 hits -- a genome-like index of 200 genomes --
  // take 7.5 ms per step in the 256-thread form and 10.3 in the 512-thread one; config 3's fragments of 3 000-4 000 hits, nine in
  // ten below the 4 096 bound, take 69.2 in the 512-thread form against 70.4 WITHOUT the pre-filter (their ~500 chance hits are
  // blocks of their own, and the 256-thread form sorts 1 024 blocks at most: what overflows takes the merge) and 60.9 against
  // 70.2 WITH it.  So: with the pre-filter the small class is kept when it holds a third of the fragments; without, when half
  // the fragments hold at most HALF its bound.  The middle class is kept from a twentieth of the fragments on (the
  // 32-hits-per-thread form behind it runs two workgroups per CU and is three times slower per fragment), or to carry the
  // small ones.  Ranges stay contiguous from 0: a wrong guess costs time, not results.
  if (p.n >= 2) {
    // S form for the small fragments, or do they ride in the middle form; the middle class stays if it has fragments of its
    // own worth a launch, or small ones to carry
    const bool keep_s = k.thin_small >= 0.0f ? (sp.l1_small_share < 0.0f || sp.l1_small_share >= k.thin_small)        // (forced: tests, A/B)
                        : sp.l1_no_small ? false
                        : p.prefilter ? (sp.l1_small_share < 0.0f || sp.l1_small_share >= 0.35f)
                                      : (sp.l1_tiny_share < 0.0f || sp.l1_tiny_share >= 0.5f);
    const bool keep_m = !keep_s || p.n == 2 || sp.l1_mid_share < 0.0f || sp.l1_mid_share >= k.thin_mid;
    L1Class c[3];
    int n = 0;
    uint32_t lo = 0u;                                            // lower bound of the next class kept
    if (keep_s) { c[n++] = p.c[0]; lo = p.c[0].n_hi + 1u; }
    if (keep_m) { c[n] = p.c[1]; c[n].n_lo = lo; lo = p.c[1].n_hi == 0xFFFFFFFFu ? lo : p.c[1].n_hi + 1u; n++; }
    if (p.n == 3) { c[n] = p.c[2]; c[n].n_lo = lo; n++; }
    for (int i = 0; i < n; i++) p.c[i] = c[i];
    p.n = n;
  }
  return p;
}

// A wave of k_l2_scan lasts as long as the longest of its 64 slides, and in k_l1's numbering it holds the loci of one fragment --
// streams of every length the divergences of the index produce (lane utilisation 85 %).  When the last accepted part had loci
// for a wave per SIMD and more, the scan takes the loci of every region sorted by stream length (profiles/r06_scan_order.txt:
// L2 stage -8 % on config 3, -9 % on config 4, -10 % on genome-like inputs and in the (16, 1000) cell, -6 % at 16 queries per
// launch, -1 % on one 5 Mb query).  FA_L2_SCAN_ORDER = 0 / 1: never / always.
inline bool scan_sorted(const Spec &sp, int knob) { return knob_or(knob, sp.l2_loci_last >= 1024 * 64); }

// Hits that cannot be an end of a candidate skip the fetch of their padded global coordinate (k_l1, scan_run<., NEAR>).  The
// hits it saves are the chance hits, whose number grows with the index (~500 per fragment at 4 x 10^8 records, ~50 at
// 4 x 10^7), and it costs a second LDS read per hit: lookup + L1 70.8 -> 67.0 ms per step on 1000 x 1000 genomes, 28.6 ->
// 28.6 on 500 x 500, 10.1 -> 10.6 on 200 x 200 (profiles/r05_l1_near_time.txt) -- so it is on from 3 x 10^8 records.
// FA_L1_NEAR = 0 / 1: never / always (the A/B of the HBM fetch: profiles/r05_l1_near_fetch.txt).
inline bool l1_near(int64_t records, int knob) { return knob_or(knob, records >= 300000000LL); }

// slot = rank + 1 must fit the slot field of the 16-bit event: larger sketches take the 32-bit events
inline bool wide_events(int smax) { return smax + 1 >= (1 << EV_RANK16); }

// Passes of several genomes (or one, FA_FRAG_ORDER_ONE) run the workgroups of k_l2_events in offset-major, XCD-aware order
// (build_frag_order) from 64 fragments on
inline bool frag_order_gate(bool on, bool one, int genomes, int64_t F) { return on && (genomes >= 2 || one) && F >= 64; }

// ------------------------------------------------------------------------------------------------------------
// the verdict on a finished part
// ------------------------------------------------------------------------------------------------------------
struct Verdict {
  enum Kind { ACCEPTED, VOIDED, SHRUNK, FAILED } kind = ACCEPTED;   // SHRUNK: void, and part_frags cut down; FAILED: F == 1 cannot shrink
  const char *what = nullptr;   // SHRUNK / FAILED: what overflowed the 32-bit offsets
  bool miss = false;            // a speculated size was too small (fa_mapper_last_timings [9], repeats)
  bool fuse_overflow = false;   // k_query_fused overflowed: the range runs again through the two kernels (fuse_overflowed)
  uint64_t loci = 0, events = 0, records = 0;   // live loci, slide events, records in the locus ranges
};

// The verdict on a part of F fragments from its status block: updates the attempt's record `sp` and says whether the part
// stands.  `loci_n` / `loci_shift`: the locus regions of the part; `items_max`: most slide events a part may address;
// `ran`: the forms it ran with; `occupancy(smax)`: workgroups per CU of the two L2 kernels at a sketch bound (0: unknown).
template <typename Occupancy>
inline Verdict judge(Spec &sp, const PassStatus &s, const Forms &ran, int64_t F, uint32_t loci_n, uint32_t loci_shift,
                     uint64_t items_max, Occupancy &&occupancy) {
  Verdict v;
  const uint64_t total_seeds = s.totals[TOT_SEEDS], max_seeds = s.totals[TOT_MAX_FRAG];
  v.events = s.pinfo[PI_EVENTS]; v.records = s.totals[TOT_RECORDS];
  uint64_t ev_region_max = 0;
  for (int i = 0; i < EV_REGIONS; i++) {
    v.events += s.ev_region[i]; v.records += s.rec_region[i];
    ev_region_max = std::max<uint64_t>(ev_region_max, s.ev_region[i]);
  }
  const unsigned long long flags = s.pinfo[PI_FLAGS] & SPEC_VOID;
  // loci: reserved per region (LociRegions); a region asked for more than it holds = SPEC_LOCI
  uint64_t loci_region_max = 0;
  for (uint32_t i = 0; i < loci_n; i++) {
    const uint64_t c = s.loci_region[i];
    loci_region_max = std::max(loci_region_max, c);
    v.loci += std::min<uint64_t>(c, 1ULL << loci_shift);
  }
  const bool wide_missed = s.counters[CNT_WIDE] > 0 && !sp.redo;   // loci overflowed the byte state, the wide pass was not launched
  v.miss = flags || wide_missed;
  // a part whose seeds / loci / slide events cannot be addressed with 32-bit offsets is cut down and run again
  auto shrink_part = [&](double have, double limit, const char *what) {
    v.what = what;
    if (F <= 1) { v.kind = Verdict::FAILED; return v; }
    sp.part_frags = std::max<int64_t>(1, std::min<int64_t>(F / 2, (int64_t)((double)F * limit / have * 0.8)));
    v.kind = Verdict::SHRUNK;
    return v;
  };
  if (total_seeds >= (1ULL << 31)) return shrink_part((double)total_seeds, 2147483648.0, "seed hits");
  // bounds for the next pass (or the repeat of this one)
  // (a multiple of 8 just above the largest sketch seen: every slot of the bound costs k_l2_scan 64 bytes of LDS per wave,
  // and on the bench workload -- largest sketch 263 -- 272 slots let nine of its workgroups share a CU where 288 let eight)
  // The first growth is that tight bound; if the workload keeps producing larger sketches (every raise voids a pass and
  // rebuilds the O(s^2) LUTs) later ones take an eighth of headroom, cut back to the largest bound that leaves k_l2_scan and
  // k_l2_events the workgroups per CU the tight bound would (occupancy).
  const int smax_seen = s.stats[STAT_SMAX];
  if (smax_seen > sp.smax) {
    const int tight = (smax_seen + 4 + 7) / 8 * 8;
    int bound = tight;
    if (sp.smax_misses > 0) {
      const int roomy = (smax_seen + smax_seen / 8 + 7) / 8 * 8;
      const int want = occupancy(tight);
      bound = want > 0 ? tight : roomy;
      for (int s2 = tight + 8; want > 0 && s2 <= roomy && occupancy(s2) == want; s2 += 8) bound = s2;
    }
    sp.smax = bound;
    sp.smax_misses++;
  }
  // LDS slots for the seed sort: a quarter of headroom over the largest fragment seen, (LDS per workgroup sets how many fragments a CU works on at once)
  const uint32_t want_slots = std::min<uint32_t>(lds_seed_cap_max(sp.smax), std::max<uint32_t>(1024, (uint32_t)((std::min<uint64_t>(max_seeds + max_seeds / 4, 1u << 30) + 255) / 256 * 256)));
  const bool slots_changed = want_slots != sp.seed_slots;
  if (flags & SPEC_SCRATCH) sp.scratch_words = std::max<uint64_t>(sp.scratch_words, s.totals[TOT_SCRATCH] + s.totals[TOT_SCRATCH] / 4);
  if (flags & SPEC_LOCI) {
    // every region has to hold its share: size the arrays for the fullest one.  A region holds the largest power of two
    // below its share of l_cap, i.e. more than half of it: twice the need is what makes the repeat fit for certain
    const int64_t need = (int64_t)(loci_region_max * loci_n);
    const int64_t want = std::max<int64_t>(sp.l_cap * 2, need * 2);
    const int64_t l_max = (1LL << 31) - 64;
    // a region holds the largest power of two below its share: at the cap that is 2^floor_log2(l_max / n), which the fullest
    // region must fit -- otherwise the repeat would overflow again at the same capacity, for ever
    const int64_t region_at_cap = (int64_t)1 << floor_log2((int)std::max<int64_t>(1, l_max / (int64_t)loci_n));
    if (need > l_max || (want >= l_max && (int64_t)loci_region_max > region_at_cap))
      return shrink_part((double)loci_region_max, (double)region_at_cap, "candidate loci");
    sp.l_cap = std::min(want, l_max);
  }
  if (flags & SPEC_QFUSE) v.fuse_overflow = true;
  if (flags & SPEC_EVENTS) {
    // every region has to hold its share: size the arena for the fullest one (the fused form reserves from one counter)
    const uint64_t need = std::max<uint64_t>(s.pinfo[PI_EVENTS], ev_region_max * ev_regions_for(F));
    if (need > items_max) return shrink_part((double)need, (double)items_max, "slide events");
    sp.items_cap = std::min<uint64_t>(items_max, std::max<uint64_t>(sp.items_cap * 2, need + need / 4));
  }
  if (flags) {                                                   // void part: run it again
    if (slots_changed && (flags & SPEC_SCRATCH)) sp.seed_slots = want_slots;
    v.kind = Verdict::VOIDED;
    return v;
  }
  if (wide_missed) { sp.redo = true; v.kind = Verdict::VOIDED; return v; }
  // fragments that do not fit the LDS slots use HBM scratch, which must exist: size it for the new slot count lazily
  if (slots_changed) sp.seed_slots = want_slots;
  sp.l2_loci_last = (int64_t)v.loci;
  if (F > 0) {
    sp.l1_small_share = (float)s.stats[STAT_SMALL] / (float)F; sp.l1_mid_share = (float)s.stats[STAT_MID] / (float)F;
    sp.l1_tiny_share = (float)s.stats[STAT_TINY] / (float)F;
  }
  // fragments whose hits were too scattered for the block sort (they took the merge, at twice the time): from one in two hundred
  // on, the passes that follow drop the hits that cannot belong to a candidate before the sort (plan_l1)
  // (with the filter on and the 256-thread class in use they are fragments whose kept chance hits -- the hashed bits keep about a
  // third of them -- still overfill that class's table of 1 365 entries: an index of 1.6 x 10^9 records leaves ~700 of 2 000, and
  // 47 % of the fragments of the 4000 x 4000 run fell back; the class is folded into the 512-thread form from then on)
  if (F > 0 && (double)s.counters[CNT_MERGED] > 0.005 * (double)F) {
    if (ran.prefilter && ran.small_class()) sp.l1_no_small = true;
    sp.l1_prefilter = true;
  }
  return v;
}

}  // namespace fa
