// fa_linkage.hip.h -- average-linkage (UPGMA) clusters of an all-vs-all hit table on the device (fa_table_linkage): rows ->
// present pairs with a fixed-point weight -> rounds that merge every mutual nearest pair of clusters -> labels.  Nothing
// here is on the mapping path: the kernels run only under that entry point, on a stream of the call's own.  The second half of
// the file keeps the merges of those rounds as a dendrogram (fa_table_dendrogram) and cuts such a list (fa_dendrogram_cut).
//
// Semantics (include/fastani_hip.h has them in full; fa_link.h the arithmetic).  A pair of genomes is present iff it exists
// after the filter of fa_table.hip.h and, with `reciprocal`, has both directions; its weight is w = rint(identity * 2^20).
// Every genome starts as a cluster labelled by its smallest member.  Two clusters with at least one present pair between
// them are a candidate, s = sum of w + qm * (|A||B| - number of present pairs), n = |A||B|; candidates are ordered by s / n
// descending -- exactly, as 128-bit cross products --, then by the smaller label, then by the larger.  The first candidate
// is merged while it has s >= qc * n.
//
// Road.  The front end is that of fa_table.hip.h; k_table_write emits its fourth form: every present pair as two directed
// entries, key from << bits | to, value (w, 1).  A round is
//   radix sort of the entries by key, reduce-by-key (sums of w and of the count: integers, so the order of the additions
//     does not matter) -- every (cluster, neighbour) once, a cluster's neighbours contiguous;
//   k_link_segments  the run of every cluster (run_ends), and the number of live entries (the one key of dropped entries
//                    sorts last);
//   k_link_best      every cluster's first candidate under the exact order, over its run as walk_runs walks it.  The
//                    partner is kept only if the candidate passes the cut-off;
//   k_link_merge     a pair that is each other's partner merges: parent[hi] = lo, the sizes add;
//   k_link_labels    label[g] = parent[label[g]];
//   k_link_relabel   both ends of every entry through parent[]; an entry inside a cluster gets the dropped key.
// The host reads {changed, live entries} once per round and stops when nothing merged.
//
// Why merging all mutual pairs at once gives the sequential result.  The order is total (no two candidates share both
// labels), so every cluster has one first candidate and the globally first candidate is mutual: a round that can merge
// does.  Average linkage is reducible: the average between a merged cluster and a third one is a weighted mean of the two
// old averages, so it is no larger than the larger of them; and under the tie rule the merged cluster carries the smaller
// label, so its candidate key is that of the old pair with the smaller label.  A mutual pair therefore stays mutual, with
// its s and n unchanged, whatever else merges, until the sequential walk reaches it.  A pair passes the cut-off or not
// independently of the rest, and no candidate that fails it can come before one that passes.
//
// Nothing races: a cluster is in at most one merge of a round, k_link_merge's thread for the smaller label is the only one
// that touches either cluster's parent and size, and every other kernel only reads what an earlier launch wrote.  No atomic
// decides anything but the `changed` epoch (an atomicMax).  The same input gives the same bytes on every run.
#pragma once

#include "fa_link.h"
#include "fa_table.hip.h"

namespace fa {

constexpr int LINK_SHORT = 32;                 // entries of a run one lane walks alone

// ---- the runs of a directed view (shared with fa_medoid.hip.h) -------------------------------------------------------------
// A directed view is `live` entries sorted by key = from << bits | to: the entries of one `from` are its run.
// Entry i < live writes its run's ends into seg_start / seg_end [n_genomes] (zeroed before) where it is the first or the last.
__device__ __forceinline__ void run_ends(const unsigned long long *keys, int32_t bits, int32_t n_genomes, int64_t i, int64_t live,
                                         int32_t *seg_start, int32_t *seg_end) {
  const uint32_t from = (uint32_t)(keys[i] >> bits);
  if (from >= (uint32_t)n_genomes) return;                          // (never: the ids were checked)
  if (i == 0 || (uint32_t)(keys[i - 1] >> bits) != from) seg_start[from] = (int32_t)i;
  if (i == live - 1 || (uint32_t)(keys[i + 1] >> bits) != from) seg_end[from] = (int32_t)(i + 1);
}

// where `key` is in the run [start, end) (sorted), or -1
__device__ __forceinline__ int32_t run_find(const unsigned long long *keys, int32_t start, int32_t end, unsigned long long key) {
  int32_t lo = start, hi = end;
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo < end && keys[lo] == key ? lo : -1;
}

// What the lane's run [start, end) accumulates (an empty run: `zero`), CALLED BY EVERY LANE OF THE WAVE.  A run of at most
// LINK_SHORT entries is walked by its own lane; the longer ones -- hubs -- one after the other by the whole wave, 64 entries
// a step, and joined across the lanes by an xor butterfly (the join must not depend on the order).  The caller supplies
//   own, from(own, owner)   what a visit needs to know of the run's lane, and how every lane gets it from lane `owner`;
//   visit(of, i, acc)       entry i of the run of a lane whose `own` is `of`, accumulated into acc;
//   join(acc, d)            acc joined with that of lane ^ d.
// Every lane reaches every shuffle: nothing in the loop over the hubs is under a lane's own condition but the last line.
template <typename Own, typename Acc, typename From, typename Visit, typename Join>
__device__ __forceinline__ Acc walk_runs(int32_t start, int32_t end, const Own &own, const Acc &zero, From from, Visit visit, Join join) {
  const int lane = threadIdx.x & 63;
  const bool is_long = end - start > LINK_SHORT;
  Acc mine = zero;
  if (!is_long)
    for (int32_t i = start; i < end; i++) visit(own, i, mine);
  unsigned long long todo = __ballot(is_long);
  while (todo) {
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1ULL;
    const int32_t s0 = __shfl(start, owner), s1 = __shfl(end, owner);
    const Own of = from(own, owner);
    Acc acc = zero;
    for (int32_t i = s0 + lane; i < s1; i += 64) visit(of, i, acc);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) join(acc, d);
    if (lane == owner) mine = acc;
  }
  return mine;
}

// one per call, zeroed before the first launch
struct LinkStatus {
  unsigned int changed;                        // the last round (1-based) in which a pair merged
  unsigned int live;                           // k_link_segments: entries of this round's directed view
  unsigned int unique;                         // reduce-by-key: distinct keys, the dropped one included
  unsigned int merges;                         // k_link_record (fa_table_dendrogram only): merge records taken so far | LINK_LOST
};
// in LinkStatus::merges, above any count (at most 2^18 - 1): k_link_record did not find a merging pair's entry in its run
constexpr unsigned int LINK_LOST = 0x80000000u;

struct LinkArgs {
  const unsigned long long *keys;      // this round's directed view: distinct keys, sorted
  const LinkSum *sums;
  int64_t bound;                       // no more than this many entries are live
  int32_t n_genomes;
  int32_t bits;                        // key = from << bits | to; the dropped key is 1 << 2 * bits
  int32_t *seg_start, *seg_end;        // [n] the run of every cluster, zeroed before k_link_segments
  int32_t *size;                       // [n] genomes of a live cluster
  int32_t *parent;                     // [n] a live cluster's own label, or what it merged into
  int32_t *best;                       // [n] the partner of the cluster's first candidate if that passes the cut-off, else -1
  int32_t *labels;                     // [n]
  unsigned long long *next_keys;       // k_link_relabel
  LinkSum *next_sums;
  long long qm, qc;
  unsigned int round;                  // 1-based
  LinkStatus *status;
};

__device__ __forceinline__ unsigned long long link_dropped(const LinkArgs &a) { return 1ULL << (2 * a.bits); }

__global__ __launch_bounds__(256) void k_link_init(LinkArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.n_genomes) return;
  a.size[g] = 1;
  a.parent[g] = (int32_t)g;
  a.labels[g] = (int32_t)g;
}

__global__ __launch_bounds__(256) void k_link_segments(LinkArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t unique = min((int64_t)a.status->unique, a.bound);
  const int64_t live = unique - (unique > 0 && a.keys[unique - 1] == link_dropped(a) ? 1 : 0);
  if (i == 0) a.status->live = (unsigned int)live;
  if (i < live) run_ends(a.keys, a.bits, a.n_genomes, i, live, a.seg_start, a.seg_end);
}

// entry i of cluster g's run as a candidate
__device__ __forceinline__ LinkCand link_candidate(const LinkArgs &a, int32_t g, int64_t i) {
  const int32_t to = (int32_t)(a.keys[i] & ((1ULL << a.bits) - 1ULL));
  LinkCand c;
  c.n = (long long)a.size[g] * (long long)a.size[to];
  c.s = link_s(a.sums[i], c.n, a.qm);
  c.lo = min(g, to); c.hi = max(g, to);
  return c;
}

__global__ __launch_bounds__(256) void k_link_best(LinkArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int32_t start = 0, end = 0;
  if (g < a.n_genomes) { start = a.seg_start[g]; end = a.seg_end[g]; }
  const LinkCand none{0, 0, 0, 0};
  const LinkCand mine = walk_runs(
      start, end, (int32_t)g, none, [&](int32_t, int owner) { return (int32_t)(g - lane + owner); },
      [&](int32_t cluster, int32_t i, LinkCand &c) {
        const LinkCand x = link_candidate(a, cluster, i);
        if (link_better(x, c)) c = x;
      },
      [](LinkCand &c, int d) {
        const LinkCand x{__shfl_xor(c.s, d), __shfl_xor(c.n, d), __shfl_xor(c.lo, d), __shfl_xor(c.hi, d)};
        if (link_better(x, c)) c = x;
      });
  if (g >= a.n_genomes) return;
  int32_t partner = -1;
  if (mine.n != 0 && link_passes(mine.s, mine.n, a.qc)) partner = mine.lo == (int32_t)g ? mine.hi : mine.lo;
  a.best[g] = partner;
}

__global__ __launch_bounds__(256) void k_link_merge(LinkArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool merged = false;
  if (g < a.n_genomes) {
    const int32_t b = a.best[g];
    if (b > (int32_t)g && b < a.n_genomes && a.best[b] == (int32_t)g) {
      a.parent[b] = (int32_t)g;
      a.size[g] += a.size[b];
      merged = true;
    }
  }
  wave_epoch(&a.status->changed, merged, a.round);
}

__global__ __launch_bounds__(256) void k_link_labels(LinkArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g < a.n_genomes) a.labels[g] = a.parent[a.labels[g]];
}

__global__ __launch_bounds__(256) void k_link_relabel(LinkArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.status->live || i >= a.bound) return;
  const unsigned long long key = a.keys[i];
  const int32_t from = a.parent[key >> a.bits], to = a.parent[key & ((1ULL << a.bits) - 1ULL)];
  a.next_keys[i] = from == to ? link_dropped(a) : (unsigned long long)from << a.bits | (unsigned long long)to;
  a.next_sums[i] = a.sums[i];
}

// ------------------------------------------------------------------------------------------------------------
// The merge list (fa_table_dendrogram) and its cuts (fa_dendrogram_cut)
// ------------------------------------------------------------------------------------------------------------
// The rounds above compute every merge of the sequential walk; k_link_record, launched between k_link_best and k_link_merge
// under fa_table_dendrogram only, keeps them.  The thread of the smaller label knows both labels and both sizes before
// k_link_merge adds them; the pair's (sum, count) of this round is the entry `to == hi` of its run, found by run_find, so
// nothing more travels through k_link_best.  A wave takes its output slots with one atomicAdd
// (ballot, popcount prefix); the slots depend on the order the waves arrive in, the result does not: the driver sorts the
// records under the order of step 4 (MergeBefore), which is total on them -- every label is absorbed once, so no two records
// share `hi` -- and which is the order the sequential walk merges in (fastani_hip.h).
__global__ __launch_bounds__(256) void k_link_record(LinkArgs a, fa_merge *merges, int64_t cap) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool merging = false;
  fa_merge m;
  m.lo = m.hi = m.size_lo = m.size_hi = 0; m.s = m.present = 0;
  if (g < a.n_genomes) {
    const int32_t b = a.best[g];
    if (b > (int32_t)g && b < a.n_genomes && a.best[b] == (int32_t)g) {
      merging = true;
      const unsigned long long key = (unsigned long long)g << a.bits | (unsigned long long)b;
      const int32_t at = run_find(a.keys, a.seg_start[g], a.seg_end[g], key);
      m.lo = (int32_t)g; m.hi = b; m.size_lo = a.size[g]; m.size_hi = a.size[b];
      // (the entry is there: b is g's partner because k_link_best read it.  Were it not, the call fails on LINK_LOST)
      if (at >= 0) {
        m.s = link_s(a.sums[at], (long long)m.size_lo * (long long)m.size_hi, a.qm);
        m.present = a.sums[at].c;
      } else {
        atomicOr(&a.status->merges, LINK_LOST);
      }
    }
  }
  const unsigned long long mask = __ballot(merging);
  if (!mask) return;                                               // (the whole wave)
  const int leader = __ffsll((long long)mask) - 1;
  int base = 0;
  if (lane == leader) base = (int)(atomicAdd(&a.status->merges, (unsigned int)__popcll(mask)) & ~LINK_LOST);
  base = __shfl(base, leader);
  const int64_t slot = (int64_t)base + __popcll(mask & ((1ULL << lane) - 1ULL));
  if (merging && slot < cap) merges[slot] = m;                     // (always: a table has at most n_genomes - 1 merges)
}

// "comes before" of step 4 on two merges
struct MergeBefore {
  __host__ __device__ bool operator()(const fa_merge &x, const fa_merge &y) const {
    return link_order(link_merge_cand(x.lo, x.hi, x.size_lo, x.size_hi, x.s), link_merge_cand(y.lo, y.hi, y.size_lo, y.size_hi, y.s)) == 1;
  }
};
// the same on the records' numbers: the sort moves 4-byte keys, not 32-byte records (which cost rocPRIM's sort kernels scratch
// memory), and k_link_gather brings the records into the order found
struct MergeIndexBefore {
  const fa_merge *merges;
  __host__ __device__ bool operator()(int32_t x, int32_t y) const { return MergeBefore()(merges[x], merges[y]); }
};

__global__ __launch_bounds__(256) void k_link_gather(const fa_merge *found, const int32_t *order, int64_t n_merges, fa_merge *sorted) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_merges) sorted[i] = found[order[i]];
}

// A cut.  The list is checked first (k_cut_check, k_cut_twice: flags, as k_table_count sets them); a `hi` that occurs twice
// is caught by scattering the merge's index to slot[hi] and reading it back in the next launch -- one of the two finds the
// other's index.  With every hi unique, slot[] is also the way from a genome to the merge that absorbs its label, so the
// forest of a cut is gathered, not scattered: parent[t][g] = lo of that merge if it passes cut t, else g (k_cut_parent).  lo <
// hi: the forest has no cycle, and a chain of parents is at most n_genomes - 1 long (a deep tree: every merge absorbs the
// label just above).  The roots are resolved by pointer jumping from one buffer into the other, bit_width(n_genomes - 1)
// rounds: after round r a pointer spans 2^r steps of the chain or ends at the root.  A round reads only what the launch before
// it wrote, so the bytes are the same on every run.
constexpr unsigned CUT_BAD_MERGE = 1u, CUT_TWICE = 2u;

struct CutStatus {
  unsigned int flags;
  unsigned int pad;
};

struct CutArgs {
  const fa_merge *merges;
  int64_t n_merges;
  int32_t n_genomes, n_cuts;
  const long long *qc;                 // [n_cuts]
  int32_t *slot;                       // [n_genomes] the merge that absorbs a label, -1 for none: all -1 before k_cut_check
  unsigned int *roots;                 // [n_cuts] zeroed before k_cut_roots
  CutStatus *status;
};

__global__ __launch_bounds__(256) void k_cut_check(CutArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (i < a.n_merges) {
    const fa_merge m = a.merges[i];
    bad = !link_merge_ok(m.lo, m.hi, m.size_lo, m.size_hi, m.s, m.present, a.n_genomes);
    if (!bad) a.slot[m.hi] = (int32_t)i;
  }
  wave_flag(&a.status->flags, bad, CUT_BAD_MERGE);
}

__global__ __launch_bounds__(256) void k_cut_twice(CutArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool twice = false;
  if (i < a.n_merges) {
    const int32_t hi = a.merges[i].hi;
    twice = hi >= 0 && hi < a.n_genomes && a.slot[hi] != (int32_t)i;       // (a bad merge wrote nothing; it has its own flag)
  }
  wave_flag(&a.status->flags, twice, CUT_TWICE);
}

// the three kernels below: blockIdx.x over the genomes, blockIdx.y strided over the cuts
__global__ __launch_bounds__(256) void k_cut_parent(CutArgs a, int32_t *parent) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.n_genomes) return;
  const int32_t i = a.slot[g];
  long long s = 0, n = 1;
  int32_t lo = (int32_t)g;
  if (i >= 0) {
    const fa_merge m = a.merges[i];
    s = m.s; n = (long long)m.size_lo * (long long)m.size_hi; lo = m.lo;
  }
  for (int32_t t = (int32_t)blockIdx.y; t < a.n_cuts; t += (int32_t)gridDim.y)
    parent[(int64_t)t * a.n_genomes + g] = i >= 0 && link_passes(s, n, a.qc[t]) ? lo : (int32_t)g;
}

__global__ __launch_bounds__(256) void k_cut_jump(const int32_t *in, int32_t *out, int32_t n_genomes, int32_t n_cuts) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n_genomes) return;
  for (int32_t t = (int32_t)blockIdx.y; t < n_cuts; t += (int32_t)gridDim.y) {
    const int32_t *row = in + (int64_t)t * n_genomes;
    out[(int64_t)t * n_genomes + g] = row[row[g]];
  }
}

__global__ __launch_bounds__(256) void k_cut_roots(CutArgs a, const int32_t *labels) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int32_t t = (int32_t)blockIdx.y; t < a.n_cuts; t += (int32_t)gridDim.y)
    wave_count(&a.roots[t], g < a.n_genomes && labels[(int64_t)t * a.n_genomes + g] == (int32_t)g);
}

}  // namespace fa
