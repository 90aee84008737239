// fa_profile.hip.h -- the per-fragment conservation profile of a mapping table on the device (fa_mappings_profile,
// fa_profile_summary): fa_hit_mapping records -> per query fragment the number of counted records, the fixed-point sum of their
// identities and the smallest of them -> per genome and threshold set the fragments, hits and sum at or above a count.  Nothing
// here is on the mapping path: the kernels run only under those two entry points, on a stream of the call's own.
//
// Semantics (include/fastani_hip.h has them in full; fa_link.h the fixed point).  Fragment f of query q is entry
// fragment_offsets[q] + f.  A record (q, f, r, identity) is counted iff identity >= min_identity in float32, and, with labels,
// query_labels[q] == reference_labels[r], and, with self_reference, self_reference[q] != r.  A counted record adds 1 to the
// entry's count and link_fixed(identity) to its sum, and lowers its `lowest` to identity.
//
// Road.
//   k_profile_check    a workgroup per chunk of PROF_CHUNK records: every id in range, every identity a non-negative number of
//                      at most 128, else the call's flags; the three filter outcomes counted, one atomic per wave and outcome;
//                      and the chunk's verdict: its one query, or -1 when it holds two.  The host reads the flags before the
//                      accumulators are touched;
//   k_profile_add      a workgroup per chunk again.  ON CHIP when the verdict names one query of at most PROF_LDS_FRAGMENTS
//                      fragments: count, 64-bit sum and 32-bit minimum of that query's fragments are kept in LDS with LDS
//                      atomics, and flushed with one global atomic per accumulator of every fragment the chunk touched.  Any
//                      other chunk -- two queries, a query of more fragments, unsorted records -- goes straight to GLOBAL
//                      atomics, three per counted record;
//   k_profile_summary  a workgroup per genome walks its fragments, threads striding, for PROF_SETS threshold sets a walk.
//
// The chunk.  The mapper emits records in (query, reference, position) order: a chunk of 8192 lies inside one query but for the
// few that straddle a boundary, and covers about five references of a 5 Mb genome, so a fragment is hit about five times on
// chip for every three global atomics.  PROF_LDS_FRAGMENTS = 4096 entries of 16 bytes are the 64 KiB a workgroup may declare
// statically: two workgroups fit the 160 KiB of a CU, and a genome of 12 Mb at the default fragment length still fits.
//
// Why the bytes do not depend on timing, on the road, or on how the records are split over calls.  Every accumulator is an
// integer -- the minimum is taken on the bit pattern of a non-negative float, which orders as the float does -- and every
// update an integer atomicAdd / atomicMin whose end value does not depend on the order of its operands; a partial result in
// LDS is the same function of fewer operands.  No float atomic anywhere.
#pragma once

#include "fa_common.h"
#include "fa_link.h"
#include "fa_table.hip.h"

namespace fa {

constexpr int PROF_THREADS = 256;
constexpr int PROF_CHUNK = 8192;                 // records per workgroup
constexpr int PROF_LDS_FRAGMENTS = 4096;         // fragments of the one query of an on-chip chunk: 16 bytes each, 64 KiB
constexpr bool PROF_POLICY_ON_CHIP = true;       // road 0: on chip wherever it fits (scripts/time_fragment_profile.py times both)
constexpr int PROF_SETS = 4;                     // threshold sets a walk of the fragments serves
constexpr unsigned PROF_BAD_QUERY = 1u, PROF_BAD_FRAGMENT = 2u, PROF_BAD_REFERENCE = 4u, PROF_BAD_IDENTITY = 8u;
constexpr unsigned PROF_INF_BITS = 0x7f800000u;  // +inf: above the bits of every identity

// one per call, zeroed before the first launch
struct ProfileStatus {
  unsigned int flags;                            // PROF_BAD_*
  unsigned int on_chip;                          // k_profile_add: workgroups that took the on-chip road
  unsigned long long counted, skipped, below;    // k_profile_check: the three filter outcomes
};

struct ProfileArgs {
  const int4 *maps;                    // the records, two int4 each
  int64_t n_maps;
  int32_t n_queries, n_references;
  const int64_t *offsets;              // [n_queries + 1]
  const int32_t *query_labels, *reference_labels, *self_reference;   // each null for none (the first two together)
  float min_identity;
  int32_t road;                        // 1 global only, 2 on chip wherever it fits
  int32_t *chunk_query;                // [chunks] k_profile_check: the chunk's one query, -1 for two
  int32_t *count;                      // the three accumulators, [offsets[n_queries]]
  unsigned long long *sum;
  unsigned int *lowest;                // the bits of a non-negative float
  ProfileStatus *status;
};

// the four fields of a record the profile reads
struct ProfileRecord { int32_t q, f, r; float identity; };
__device__ __forceinline__ ProfileRecord profile_record(const int4 *maps, int64_t i) {
  const int4 head = maps[2 * i], tail = maps[2 * i + 1];
  return ProfileRecord{head.x, head.y, head.z, __int_as_float(tail.w)};
}

// What both profiles ask of a record -- this one and the reference-side one of fa_refprofile.hip.h, whose argument block has
// the same n_queries, n_references, labels, self_reference and min_identity -- is written once, in the two functions below.
// PROF_BAD_QUERY, PROF_BAD_REFERENCE and PROF_BAD_IDENTITY of a record, 0 for none
template <typename Args>
__device__ __forceinline__ unsigned int profile_faults(const Args &a, const ProfileRecord &m) {
  unsigned int bad = 0;
  if ((uint32_t)m.q >= (uint32_t)a.n_queries) bad |= PROF_BAD_QUERY;
  if ((uint32_t)m.r >= (uint32_t)a.n_references) bad |= PROF_BAD_REFERENCE;
  // a number in [+0, 128]: the bits of such a float are at most those of 128 (a set sign bit and every NaN lie above)
  if ((uint32_t)__float_as_int(m.identity) > 0x43000000u) bad |= PROF_BAD_IDENTITY;
  return bad;
}

// 0 counted, 1 dropped by labels or self, 2 below min_identity (which is asked first); the ids of `m` are in range
template <typename Args>
__device__ __forceinline__ int profile_outcome(const Args &a, const ProfileRecord &m) {
  if (!(m.identity >= a.min_identity)) return 2;
  if (a.query_labels && a.query_labels[m.q] != a.reference_labels[m.r]) return 1;
  if (a.self_reference && a.self_reference[m.q] == m.r) return 1;
  return 0;
}

__device__ __forceinline__ void wave_count64(unsigned long long *count, unsigned int mine) {           // *count += the sum over the lanes
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, (unsigned long long)mine);
}

__global__ __launch_bounds__(PROF_THREADS) void k_profile_check(ProfileArgs a) {
  __shared__ int mixed;
  const int64_t lo = (int64_t)blockIdx.x * PROF_CHUNK, hi = lo + PROF_CHUNK < a.n_maps ? lo + PROF_CHUNK : a.n_maps;
  if (threadIdx.x == 0) mixed = 0;
  __syncthreads();
  const int32_t q0 = profile_record(a.maps, lo).q;               // (lo < n_maps: the grid has no empty chunk)
  unsigned int flags = 0, n[3] = {0, 0, 0};
  bool other = false;
  for (int64_t i = lo + threadIdx.x; i < hi; i += PROF_THREADS) {
    const ProfileRecord m = profile_record(a.maps, i);
    other |= m.q != q0;
    unsigned int bad = profile_faults(a, m);
    if (!(bad & PROF_BAD_QUERY) && (m.f < 0 || (int64_t)m.f >= a.offsets[m.q + 1] - a.offsets[m.q])) bad |= PROF_BAD_FRAGMENT;
    flags |= bad;
    if (!bad) {
      const int o = profile_outcome(a, m);
      n[0] += o == 0; n[1] += o == 1; n[2] += o == 2;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) flags |= __shfl_xor(flags, d);
  if ((threadIdx.x & 63) == 0 && flags) atomicOr(&a.status->flags, flags);
  wave_count64(&a.status->counted, n[0]);
  wave_count64(&a.status->skipped, n[1]);
  wave_count64(&a.status->below, n[2]);
  if (other) mixed = 1;                                           // (every writer writes the same value)
  __syncthreads();
  if (threadIdx.x == 0) a.chunk_query[blockIdx.x] = mixed ? -1 : q0;
}

// the records have passed k_profile_check: every index below is in range
__global__ __launch_bounds__(PROF_THREADS) void k_profile_add(ProfileArgs a) {
  __shared__ unsigned long long l_sum[PROF_LDS_FRAGMENTS];
  __shared__ int l_count[PROF_LDS_FRAGMENTS];
  __shared__ unsigned int l_lowest[PROF_LDS_FRAGMENTS];
  const int64_t lo = (int64_t)blockIdx.x * PROF_CHUNK, hi = lo + PROF_CHUNK < a.n_maps ? lo + PROF_CHUNK : a.n_maps;
  const int32_t q = a.chunk_query[blockIdx.x];
  int64_t base = 0, fragments = 0;
  if (q >= 0) { base = a.offsets[q]; fragments = a.offsets[q + 1] - base; }
  const bool on_chip = a.road != 1 && q >= 0 && fragments <= (int64_t)PROF_LDS_FRAGMENTS;          // (uniform over the workgroup)
  if (!on_chip) {
    for (int64_t i = lo + threadIdx.x; i < hi; i += PROF_THREADS) {
      const ProfileRecord m = profile_record(a.maps, i);
      if (profile_outcome(a, m) != 0) continue;
      const int64_t at = a.offsets[m.q] + m.f;
      atomicAdd(a.count + at, 1);
      atomicAdd(a.sum + at, (unsigned long long)link_fixed((double)m.identity));
      atomicMin(a.lowest + at, (unsigned int)__float_as_int(m.identity));
    }
    return;
  }
  const int n = (int)fragments;
  for (int f = threadIdx.x; f < n; f += PROF_THREADS) { l_sum[f] = 0ULL; l_count[f] = 0; l_lowest[f] = PROF_INF_BITS; }
  __syncthreads();
  for (int64_t i = lo + threadIdx.x; i < hi; i += PROF_THREADS) {
    const ProfileRecord m = profile_record(a.maps, i);
    if (profile_outcome(a, m) != 0) continue;
    atomicAdd(&l_count[m.f], 1);
    atomicAdd(&l_sum[m.f], (unsigned long long)link_fixed((double)m.identity));
    atomicMin(&l_lowest[m.f], (unsigned int)__float_as_int(m.identity));
  }
  __syncthreads();
  for (int f = threadIdx.x; f < n; f += PROF_THREADS) {
    const int c = l_count[f];
    if (!c) continue;
    atomicAdd(a.count + base + f, c);
    atomicAdd(a.sum + base + f, l_sum[f]);
    atomicMin(a.lowest + base + f, l_lowest[f]);
  }
  if (threadIdx.x == 0) atomicAdd(&a.status->on_chip, 1u);
}

struct SummaryArgs {
  const int32_t *count;                // the profile, [offsets[n_queries]]
  const long long *sum;
  const int64_t *offsets;              // [n_queries + 1]
  const int32_t *min_count;            // [n_sets][n_queries]
  int32_t n_queries, n_sets;
  int64_t *fragments, *hits, *sums;    // the outputs, each [n_sets][n_queries] or null
};

// blockIdx.x: the genome; blockIdx.y strided over groups of PROF_SETS sets
__global__ __launch_bounds__(PROF_THREADS) void k_profile_summary(SummaryArgs a) {
  __shared__ long long part[PROF_THREADS / 64][PROF_SETS][3];
  const int32_t q = (int32_t)blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t lo = a.offsets[q], hi = a.offsets[q + 1];
  for (int32_t t0 = (int32_t)blockIdx.y * PROF_SETS; t0 < a.n_sets; t0 += (int32_t)gridDim.y * PROF_SETS) {
    int32_t need[PROF_SETS];
    long long acc[PROF_SETS][3] = {};
#pragma unroll
    for (int u = 0; u < PROF_SETS; u++) need[u] = t0 + u < a.n_sets ? a.min_count[(int64_t)(t0 + u) * a.n_queries + q] : INT32_MAX;
    for (int64_t i = lo + threadIdx.x; i < hi; i += PROF_THREADS) {
      const int32_t c = a.count[i];
      const long long s = a.sum[i];
#pragma unroll
      for (int u = 0; u < PROF_SETS; u++)
        if (t0 + u < a.n_sets && c >= need[u]) { acc[u][0] += 1; acc[u][1] += c; acc[u][2] += s; }
    }
#pragma unroll
    for (int u = 0; u < PROF_SETS; u++)
#pragma unroll
      for (int k = 0; k < 3; k++) {
        long long v = acc[u][k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        if (lane == 0) part[wave][u][k] = v;
      }
    __syncthreads();
    if (threadIdx.x < PROF_SETS * 3) {
      const int u = threadIdx.x / 3, k = threadIdx.x % 3;
      if (t0 + u < a.n_sets) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < PROF_THREADS / 64; w++) v += part[w][u][k];
        int64_t *out = k == 0 ? a.fragments : k == 1 ? a.hits : a.sums;
        if (out) out[(int64_t)(t0 + u) * a.n_queries + q] = (int64_t)v;
      }
    }
    __syncthreads();
  }
}

}  // namespace fa
