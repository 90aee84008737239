// fa_linkage.hip.h -- average-linkage (UPGMA) clusters of an all-vs-all hit table on the device (fa_table_linkage): rows ->
// present pairs with a fixed-point weight -> rounds that merge every mutual nearest pair of clusters -> labels.  Nothing
// here is on the mapping path: the kernels run only under that entry point, on a stream of the call's own.
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
//   k_link_segments  the run of every cluster, and the number of live entries (the one key of dropped entries sorts last);
//   k_link_best      every cluster's first candidate under the exact order: one lane per run of at most LINK_SHORT
//                    entries; a longer run -- a hub -- is walked by the whole wave, 64 entries a step, and reduced
//                    across the lanes.  The partner is kept only if the candidate passes the cut-off;
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

// one per call, zeroed before the first launch
struct LinkStatus {
  unsigned int changed;                        // the last round (1-based) in which a pair merged
  unsigned int live;                           // k_link_segments: entries of this round's directed view
  unsigned int unique;                         // reduce-by-key: distinct keys, the dropped one included
  unsigned int pad;
};

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
  if (i >= live) return;
  const uint32_t from = (uint32_t)(a.keys[i] >> a.bits);
  if (from >= (uint32_t)a.n_genomes) return;                        // (never: the ids were checked)
  if (i == 0 || (uint32_t)(a.keys[i - 1] >> a.bits) != from) a.seg_start[from] = (int32_t)i;
  if (i == live - 1 || (uint32_t)(a.keys[i + 1] >> a.bits) != from) a.seg_end[from] = (int32_t)(i + 1);
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
  LinkCand mine;
  mine.s = 0; mine.n = 0; mine.lo = 0; mine.hi = 0;
  const bool is_long = end - start > LINK_SHORT;
  if (!is_long)
    for (int32_t i = start; i < end; i++) {
      const LinkCand c = link_candidate(a, (int32_t)g, i);
      if (link_better(c, mine)) mine = c;
    }
  // the long runs of this wave's clusters, one after the other, by all of its lanes
  unsigned long long todo = __ballot(is_long);
  while (todo) {
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1ULL;
    const int32_t cluster = (int32_t)(g - lane + owner);
    const int32_t s0 = __shfl(start, owner), s1 = __shfl(end, owner);
    LinkCand c;
    c.s = 0; c.n = 0; c.lo = 0; c.hi = 0;
    for (int32_t i = s0 + lane; i < s1; i += 64) {
      const LinkCand x = link_candidate(a, cluster, i);
      if (link_better(x, c)) c = x;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      LinkCand x;
      x.s = __shfl_xor(c.s, d); x.n = __shfl_xor(c.n, d); x.lo = __shfl_xor(c.lo, d); x.hi = __shfl_xor(c.hi, d);
      if (link_better(x, c)) c = x;
    }
    if (lane == owner) mine = c;
  }
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
  const unsigned long long m = __ballot(merged);                   // one atomicMax per wave that merged a pair
  if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicMax(&a.status->changed, a.round);
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

}  // namespace fa
