// fa_medoid.hip.h -- centrality and medoids of the clusters of an all-vs-all hit table on the device (fa_table_medoids): rows ->
// present pairs with a fixed-point weight -> every genome's sum over its own cluster -> the member with the largest sum per
// cluster -> every member's identity to it.  Nothing here is on the mapping path: the kernels run only under that entry point,
// on a stream of the call's own.
//
// Semantics (include/fastani_hip.h has them in full; fa_link.h the arithmetic).  The partition is the caller's: n_sets label
// sets over the same genomes, labels[t][g] a member of g's cluster that labels itself.  For a member g of a cluster of m
//     S = sum of w over the present pairs (g, h), h in the cluster + qm * (m - 1 - their number),     T = S + qb[g] * (m - 1);
// the medoid of the cluster is its member with the largest T, ties to the smaller genome number.
//
// Road.  The front end is that of fa_table.hip.h; k_table_write emits its fourth form, every present pair as two directed
// entries, key from << bits | to, value (w, 1), as for fa_linkage.hip.h.  Then
//   k_medoid_check     one thread per (set, genome): the label lies in [0, n) and labels itself, else the call's flag; a good
//                      label's slot counts the genome (atomicAdd): size[t][label] = m;
//   radix sort of the entries by key, ONCE for all the sets -- a genome's neighbours contiguous and ascending;
//   k_medoid_segments  the run of every genome (run_ends of fa_linkage.hip.h);
//   k_medoid_sums      every genome's (sum of w, count) over the entries whose other end carries its label, for MED_SETS label
//                      sets at a time, over its run as walk_runs (fa_linkage.hip.h) walks it.  It writes S;
//   k_medoid_best      atomicMax of medoid_key(T) into the slot of the label;
//   k_medoid_pick      atomicMin of the genome number, among the members whose key is the slot's, into a second slot;
//   k_medoid_write     the medoid of every genome's cluster, the weight of the entry (g, medoid) of g's run (run_find) -- or
//                      NaN --, S and m; a wave counts the genomes that are their own medoid (wave_count).
//
// Why the bytes do not depend on timing.  Every sum is a sum of integers, taken by one lane or one wave in a fixed order.
// Every cross-workgroup effect is an integer atomicAdd / atomicMax / atomicMin / atomicOr into a slot zeroed (or filled)
// before the launch, whose end value does not depend on the order of its operands, and every slot is read only by a later
// launch.  T and a genome number do not fit one 64-bit key together, hence the two steps: the largest key first, then the
// smallest number among those that reach it -- the relation medoid_better of fa_link.h.
#pragma once

#include "fa_link.h"
#include "fa_linkage.hip.h"

namespace fa {

constexpr int MED_SETS = 4;                    // label sets a walk of the entries serves
constexpr unsigned MED_BAD_LABEL = 1u;
constexpr unsigned long long MED_NAN = 0x7ff8000000000000ULL;       // the NaN of an identity that has no row

// one per call, zeroed before the first launch
struct MedoidStatus {
  unsigned int flags;                          // MED_BAD_LABEL
  unsigned int pad;
  unsigned long long inside;                   // k_medoid_sums: directed entries inside a cluster, over all sets
};

struct MedoidArgs {
  const unsigned long long *keys;      // the directed entries, sorted
  const LinkSum *sums;
  int64_t n_entries;
  int32_t n_genomes, n_sets;
  int32_t bits;                        // key = from << bits | to
  const int32_t *labels;               // [n_sets][n]
  int32_t *seg_start, *seg_end;        // [n] the run of every genome, zeroed before k_medoid_segments
  int32_t *size;                       // [n_sets][n] at a label's slot: the genomes that carry it; zeroed before k_medoid_check
  long long *s;                        // [n_sets][n] S of every genome
  const long long *qb;                 // [n], or null for no bonus
  unsigned long long *best;            // [n_sets][n] at a label's slot: the largest medoid_key; zeroed before k_medoid_best
  int32_t *who;                        // [n_sets][n] at a label's slot: the medoid; above every genome number before k_medoid_pick
  long long qm;
  int32_t *medoids;                    // the four outputs, each [n_sets][n] or null
  double *identity;
  int64_t *sums_out;
  int32_t *sizes_out;
  unsigned int *roots;                 // [n_sets] zeroed before k_medoid_write
  MedoidStatus *status;
};

// the kernels over (set, genome): blockIdx.x over the genomes, blockIdx.y strided over the sets
__global__ __launch_bounds__(256) void k_medoid_check(MedoidArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int32_t t = (int32_t)blockIdx.y; t < a.n_sets; t += (int32_t)gridDim.y) {
    const int32_t *row = a.labels + (int64_t)t * a.n_genomes;
    bool bad = false;
    if (g < a.n_genomes) {
      const int32_t l = row[g];
      bad = (uint32_t)l >= (uint32_t)a.n_genomes || row[l] != l;
      if (!bad) atomicAdd(a.size + (int64_t)t * a.n_genomes + l, 1);
    }
    wave_flag(&a.status->flags, bad, MED_BAD_LABEL);
  }
}

__global__ __launch_bounds__(256) void k_medoid_segments(MedoidArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.n_entries) run_ends(a.keys, a.bits, a.n_genomes, i, a.n_entries, a.seg_start, a.seg_end);
}

// what walk_runs carries for k_medoid_sums: a genome's labels in MED_SETS sets; (sum of w, count) of the entries that match them
struct MedoidOwn { int32_t label[MED_SETS]; };
struct MedoidAcc { long long w[MED_SETS] = {}; int32_t c[MED_SETS] = {}; };

// blockIdx.y strided over groups of MED_SETS sets
__global__ __launch_bounds__(256) void k_medoid_sums(MedoidArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = g < a.n_genomes;
  const int64_t n = a.n_genomes;
  int32_t start = 0, end = 0;
  if (live) { start = a.seg_start[g]; end = a.seg_end[g]; }
  const unsigned long long to_mask = (1ULL << a.bits) - 1ULL;
  unsigned long long inside = 0;
  for (int32_t t0 = (int32_t)blockIdx.y * MED_SETS; t0 < a.n_sets; t0 += (int32_t)gridDim.y * MED_SETS) {
    MedoidOwn own;
#pragma unroll
    for (int u = 0; u < MED_SETS; u++)
      own.label[u] = live && t0 + u < a.n_sets ? a.labels[(int64_t)(t0 + u) * n + g] : -1;      // (-1: no label is negative)
    const MedoidAcc sum = walk_runs(
        start, end, own, MedoidAcc{}, [](const MedoidOwn &o, int owner) {
          MedoidOwn x;
#pragma unroll
          for (int u = 0; u < MED_SETS; u++) x.label[u] = __shfl(o.label[u], owner);
          return x;
        },
        [&](const MedoidOwn &of, int32_t i, MedoidAcc &acc) {
          const int64_t to = (int64_t)(a.keys[i] & to_mask);
          const long long wi = a.sums[i].w;
#pragma unroll
          for (int u = 0; u < MED_SETS; u++)
            if (t0 + u < a.n_sets && a.labels[(int64_t)(t0 + u) * n + to] == of.label[u]) { acc.w[u] += wi; acc.c[u]++; }
        },
        [](MedoidAcc &acc, int d) {
#pragma unroll
          for (int u = 0; u < MED_SETS; u++) { acc.w[u] += __shfl_xor(acc.w[u], d); acc.c[u] += __shfl_xor(acc.c[u], d); }
        });
#pragma unroll
    for (int u = 0; u < MED_SETS; u++) {
      if (own.label[u] < 0) continue;
      const int64_t at = (int64_t)(t0 + u) * n;
      a.s[at + g] = medoid_s(sum.w[u], sum.c[u], a.size[at + own.label[u]], a.qm);
      inside += (unsigned long long)sum.c[u];
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) inside += __shfl_xor(inside, d);
  if (lane == 0 && inside) atomicAdd(&a.status->inside, inside);
}

// T of genome g in set t and the slot of its label
__device__ __forceinline__ long long medoid_own_t(const MedoidArgs &a, int32_t t, int64_t g, int64_t &slot) {
  const int64_t at = (int64_t)t * a.n_genomes;
  slot = at + a.labels[at + g];
  return medoid_t(a.s[at + g], a.qb ? a.qb[g] : 0, a.size[slot]);
}

__global__ __launch_bounds__(256) void k_medoid_best(MedoidArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.n_genomes) return;
  for (int32_t t = (int32_t)blockIdx.y; t < a.n_sets; t += (int32_t)gridDim.y) {
    int64_t slot;
    const long long own = medoid_own_t(a, t, g, slot);
    atomicMax(a.best + slot, medoid_key(own));
  }
}

__global__ __launch_bounds__(256) void k_medoid_pick(MedoidArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.n_genomes) return;
  for (int32_t t = (int32_t)blockIdx.y; t < a.n_sets; t += (int32_t)gridDim.y) {
    int64_t slot;
    const long long own = medoid_own_t(a, t, g, slot);
    if (medoid_key(own) == a.best[slot]) atomicMin(a.who + slot, (int32_t)g);
  }
}

__global__ __launch_bounds__(256) void k_medoid_write(MedoidArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int32_t t = (int32_t)blockIdx.y; t < a.n_sets; t += (int32_t)gridDim.y) {
    bool root = false;
    if (g < a.n_genomes) {
      const int64_t at = (int64_t)t * a.n_genomes;
      const int64_t slot = at + a.labels[at + g];
      const int32_t medoid = a.who[slot];
      root = medoid == (int32_t)g;
      if (a.medoids) a.medoids[at + g] = medoid;
      if (a.sums_out) a.sums_out[at + g] = (int64_t)a.s[at + g];
      if (a.sizes_out) a.sizes_out[at + g] = a.size[slot];
      if (a.identity) {
        double identity = 100.0;
        if (!root) {
          // (medoid < n_genomes: the slot's own genome reaches the slot's largest key at the latest)
          const unsigned long long key = (unsigned long long)g << a.bits | (unsigned long long)(uint32_t)medoid;
          const int32_t at = run_find(a.keys, a.seg_start[g], a.seg_end[g], key);
          identity = at >= 0 ? (double)a.sums[at].w / LINK_SCALE : __longlong_as_double((long long)MED_NAN);
        }
        a.identity[at + g] = identity;
      }
    }
    wave_count(&a.roots[t], root);
  }
}

}  // namespace fa
