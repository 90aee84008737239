// fa_refprofile.hip.h -- the reference side of the conservation profile, and the regions of either profile
// (fa_mappings_reference_profile, fa_profile_regions): fa_hit_mapping records -> per reference bin the number of counted
// records, the fixed-point sum of their identities and the smallest of them; a profile's count (and sum) -> the maximal runs
// of entries at or above, or below, a presence threshold, per contig, in order.  Nothing here is on the mapping path: the
// kernels run only under those two entry points, on a stream of the call's own.
//
// Semantics (include/fastani_hip.h has them in full; fa_link.h the fixed point).  A record (q, r, contig c, position p,
// identity) goes to entry contig_bin[c] + p / bin_length, the bin computeCGI kept it for (cgi_survivor, fa_map.hip.h).  What
// is counted is what fa_mappings_profile counts: the two profiles share profile_faults and profile_outcome
// (fa_profile.hip.h), and this file adds only the three faults of a reference position.
//
// Road of the profile.
//   k_refprofile_check  a workgroup per chunk of REFPROF_CHUNK records: every id in range, the contig one of the record's
//                       reference genome, the position inside the contig's bins, every identity a non-negative number of at
//                       most 128, else the call's flags; the three filter outcomes counted, one atomic per wave and outcome.
//                       The host reads the flags before the accumulators are touched;
//   k_refprofile_add    a workgroup per chunk again: three global integer atomics per counted record.
// There is no on-chip road, unlike k_profile_add.  The mapper emits records in (query, reference genome, bin) order with at
// most one record per (query, reference genome, bin), so the records of one workgroup's chunk fall on DISTINCT bins: a
// partial sum in LDS would hold one operand per entry and save nothing.  The operands that meet on a bin come from
// different queries, a genome's worth of records apart in the stream.  What the order does give is the shape of the
// atomics: consecutive lanes hold consecutive records, hence consecutive bins, so a wave's atomic instruction on `count` or
// `lowest` covers 256 contiguous bytes, and 512 on `sum` -- the shape the programming guide's Guideline 12 ("shape each
// atomic wave-instruction as 256 contiguous bytes ... spread the adds over many rows") asks for.
// REFPROF_THREADS = 256 is Guideline 11's block ("a multiple of 64; 256 is a common default"); REFPROF_CHUNK = 8192, 32
// records a thread, is k_profile_add's chunk, so that the timing beside its global-atomics road
// (scripts/time_reference_profile.py) compares the addressing and nothing else, and gives the 6.7e7 records of a
// 200 x 200 all-vs-all some 8 000 workgroups, about four waves of workgroups over the chip's 256 CUs at eight a CU.
//
// Why the bytes do not depend on timing or on how the records are split over calls: as in fa_profile.hip.h, every
// accumulator is an integer (the minimum is taken on the bit pattern of a non-negative float) and every update an integer
// atomicAdd / atomicMin.  No float atomic anywhere.
//
// Road of the regions: an ordered compaction like every other of the library (count per chunk, k_chunk_scan of
// fa_compact.hip.h, write), twice.
//   k_region_runs<false>  a workgroup per chunk of REG_CHUNK entries: an entry HOLDS iff count >= need[its segment] (with
//                         `below`: count < need); it STARTS a run when it holds and is its segment's first entry or its
//                         predecessor does not hold, and ENDS one when it holds and is the segment's last or its successor
//                         does not.  The chunk's starts and ends are counted; the segment of an entry is found by bisection
//                         of the offsets;
//   k_chunk_scan          over the starts and over the ends;
//   k_region_runs<true>   the k-th start writes (segment, entry) to run k, the k-th end its entry: runs do not overlap, so
//                         ends come in the order of starts and no lane ever walks a run;
//   k_region_emit<false>  a workgroup per chunk of REG_CHUNK runs counts those of at least min_length entries;
//   k_chunk_scan, then    k_region_emit<true> writes them as records.  hits and sum are differences of rocPRIM exclusive
//                         scans of count and sum over the whole profile (every entry of a run holds, so no mask is needed;
//                         the scans are unsigned 64-bit, and a difference is exact modulo 2^64 whatever the prefix reached).
// A record's place is a function of the entries alone: the same input gives the same bytes on every run.  Worst case: 16
// bytes of scratch per entry for the two scans, 12 per run; time linear in the entries, log2(n_segments) reads an entry for
// the bisection.
#pragma once

#include <rocprim/rocprim.hpp>

#include "fa_common.h"
#include "fa_compact.hip.h"
#include "fa_link.h"
#include "fa_profile.hip.h"

namespace fa {

constexpr int REFPROF_THREADS = 256;
constexpr int REFPROF_CHUNK = 8192;              // records per workgroup
constexpr unsigned PROF_BAD_CONTIG = 16u, PROF_BAD_CONTIG_GENOME = 32u, PROF_BAD_POSITION = 64u;   // beside PROF_BAD_* of fa_profile.hip.h

struct RefProfileArgs {
  const int4 *maps;                    // the records, two int4 each
  int64_t n_maps;
  int32_t n_queries, n_references, n_contigs;
  const int32_t *contig_bin;           // [n_contigs + 1]
  const int32_t *contig_genome;        // [n_contigs]
  int32_t bin_length;
  const int32_t *query_labels, *reference_labels, *self_reference;   // each null for none (the first two together)
  float min_identity;
  int32_t *count;                      // the three accumulators, [contig_bin[n_contigs]]
  unsigned long long *sum;
  unsigned int *lowest;                // the bits of a non-negative float
  ProfileStatus *status;               // (on_chip stays 0)
};

// a record as the reference side reads it: the fields both profiles read, the contig and the position on it
struct RefProfileRecord { ProfileRecord m; int32_t contig, position; };
__device__ __forceinline__ RefProfileRecord refprofile_record(const int4 *maps, int64_t i) {
  const int4 head = maps[2 * i], tail = maps[2 * i + 1];
  return RefProfileRecord{ProfileRecord{head.x, head.y, head.z, __int_as_float(tail.w)}, head.w, tail.x};
}

__global__ __launch_bounds__(REFPROF_THREADS) void k_refprofile_check(RefProfileArgs a) {
  const int64_t lo = (int64_t)blockIdx.x * REFPROF_CHUNK, hi = lo + REFPROF_CHUNK < a.n_maps ? lo + REFPROF_CHUNK : a.n_maps;
  unsigned int flags = 0, n[3] = {0, 0, 0};
  for (int64_t i = lo + threadIdx.x; i < hi; i += REFPROF_THREADS) {
    const RefProfileRecord rec = refprofile_record(a.maps, i);
    unsigned int bad = profile_faults(a, rec.m);
    if ((uint32_t)rec.contig >= (uint32_t)a.n_contigs) bad |= PROF_BAD_CONTIG;
    else {
      if (a.contig_genome[rec.contig] != rec.m.r) bad |= PROF_BAD_CONTIG_GENOME;
      const int64_t bins = (int64_t)a.contig_bin[rec.contig + 1] - a.contig_bin[rec.contig];
      if (rec.position < 0 || (int64_t)(rec.position / a.bin_length) >= bins) bad |= PROF_BAD_POSITION;
    }
    flags |= bad;
    if (!bad) {
      const int o = profile_outcome(a, rec.m);
      n[0] += o == 0; n[1] += o == 1; n[2] += o == 2;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) flags |= __shfl_xor(flags, d);
  if ((threadIdx.x & 63) == 0 && flags) atomicOr(&a.status->flags, flags);
  wave_count64(&a.status->counted, n[0]);
  wave_count64(&a.status->skipped, n[1]);
  wave_count64(&a.status->below, n[2]);
}

// the records have passed k_refprofile_check: every index below is in range
__global__ __launch_bounds__(REFPROF_THREADS) void k_refprofile_add(RefProfileArgs a) {
  const int64_t lo = (int64_t)blockIdx.x * REFPROF_CHUNK, hi = lo + REFPROF_CHUNK < a.n_maps ? lo + REFPROF_CHUNK : a.n_maps;
  for (int64_t i = lo + threadIdx.x; i < hi; i += REFPROF_THREADS) {
    const RefProfileRecord rec = refprofile_record(a.maps, i);
    if (profile_outcome(a, rec.m) != 0) continue;
    const int64_t at = (int64_t)a.contig_bin[rec.contig] + rec.position / a.bin_length;
    atomicAdd(a.count + at, 1);
    atomicAdd(a.sum + at, (unsigned long long)link_fixed((double)rec.m.identity));
    atomicMin(a.lowest + at, (unsigned int)__float_as_int(rec.m.identity));
  }
}

// ---- regions -----------------------------------------------------------------------------------------------------------
constexpr int REG_THREADS = 256;
constexpr int REG_ITERS = 8, REG_CHUNK = REG_THREADS * REG_ITERS;   // entries (and, in k_region_emit, runs) per workgroup

// the header's fa_profile_region, word for word
struct RegionRecord { int32_t segment, first, length, reserved; long long hits, sum; };
static_assert(sizeof(RegionRecord) == 32 && sizeof(fa_profile_region) == 32, "a region record is 32 bytes");

// one per call, zeroed before the first launch: the totals of the three scans
struct RegionStatus { int64_t starts, ends, regions; };

struct RegionArgs {
  const int32_t *count;                // the profile, [total]
  const unsigned long long *sum;       // null: every record's sum is 0
  const int64_t *offsets;              // [n_segments + 1]
  const int32_t *need;                 // [n_segments]
  int32_t n_segments, total, below, min_length;
  int32_t *chunk_starts, *chunk_ends;  // [chunks of entries]
  int64_t *start_off, *end_off;
  int32_t *run_segment, *run_first, *run_last;     // [n_runs]: a run's segment, its first and its last entry
  int64_t n_runs;
  int32_t *chunk_kept;                 // [chunks of runs]
  int64_t *kept_off;
  const unsigned long long *count_before, *sum_before;   // [total]: the exclusive sums of count and of sum
  RegionRecord *regions;
};

struct RegionEntry { int32_t segment; bool start, end; };
// entry i of the profile, 0 <= i < total
__device__ __forceinline__ RegionEntry region_entry(const RegionArgs &a, int32_t i) {
  // the segment that holds i: offsets[lo] <= i < offsets[hi] throughout (offsets[0] == 0, offsets[n_segments] == total), so the
  // answer is never an empty segment
  int32_t lo = 0, hi = a.n_segments;
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (a.offsets[mid] <= (int64_t)i) lo = mid; else hi = mid;
  }
  const int32_t need = a.need[lo];
  const bool below = a.below != 0;
  RegionEntry e{lo, false, false};
  if ((a.count[i] >= need) == below) return e;                                      // does not hold
  e.start = (int64_t)i == a.offsets[lo] || (a.count[i - 1] >= need) == below;
  e.end = (int64_t)i + 1 == a.offsets[lo + 1] || (a.count[i + 1] >= need) == below;
  return e;
}

// One trip of a workgroup's ordered compaction, CALLED BY EVERY THREAD: returns the flagged threads of the trip ahead of this
// one, and adds the trip's flagged threads to `total`.  `sh` holds an int for each wave.
__device__ __forceinline__ int trip_rank(bool flag, int *sh, int &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  if (lane == 0) sh[wave] = __popcll(m);
  __syncthreads();
  int ahead = __popcll(m & ((1ULL << lane) - 1ULL));
#pragma unroll
  for (int w = 0; w < REG_THREADS / 64; w++) {
    const int n = sh[w];
    if (w < wave) ahead += n;
    total += n;
  }
  __syncthreads();
  return ahead;
}

// WRITE false: the starts and the ends of chunk blockIdx.x counted; true: written to their runs
template <bool WRITE>
__global__ __launch_bounds__(REG_THREADS) void k_region_runs(RegionArgs a) {
  __shared__ int sh[REG_THREADS / 64];
  const int64_t lo = (int64_t)blockIdx.x * REG_CHUNK;
  int starts = 0, ends = 0;                                        // of the trips so far (uniform over the workgroup)
  for (int it = 0; it < REG_ITERS; it++) {
    const int64_t i = lo + (int64_t)it * REG_THREADS + threadIdx.x;
    RegionEntry e{0, false, false};
    if (i < (int64_t)a.total) e = region_entry(a, (int32_t)i);
    const int start_base = starts, end_base = ends;
    const int start_rank = trip_rank(e.start, sh, starts), end_rank = trip_rank(e.end, sh, ends);
    if (WRITE) {
      if (e.start) {
        const int64_t k = a.start_off[blockIdx.x] + start_base + start_rank;
        a.run_segment[k] = e.segment;
        a.run_first[k] = (int32_t)i;
      }
      if (e.end) a.run_last[a.end_off[blockIdx.x] + end_base + end_rank] = (int32_t)i;
    }
  }
  if (!WRITE && threadIdx.x == 0) { a.chunk_starts[blockIdx.x] = starts; a.chunk_ends[blockIdx.x] = ends; }
}

// over the runs.  WRITE false: those of at least min_length entries counted per chunk; true: written as records
template <bool WRITE>
__global__ __launch_bounds__(REG_THREADS) void k_region_emit(RegionArgs a) {
  __shared__ int sh[REG_THREADS / 64];
  const int64_t lo = (int64_t)blockIdx.x * REG_CHUNK;
  int kept = 0;
  for (int it = 0; it < REG_ITERS; it++) {
    const int64_t k = lo + (int64_t)it * REG_THREADS + threadIdx.x;
    int32_t first = 0, last = -1;
    if (k < a.n_runs) { first = a.run_first[k]; last = a.run_last[k]; }
    const bool keep = k < a.n_runs && last - first + 1 >= a.min_length;
    const int base = kept;
    const int rank = trip_rank(keep, sh, kept);
    if (WRITE && keep) {
      const int32_t s = a.run_segment[k];
      RegionRecord r;
      r.segment = s; r.first = (int32_t)((int64_t)first - a.offsets[s]); r.length = last - first + 1; r.reserved = 0;
      r.hits = (long long)(a.count_before[last] - a.count_before[first] + (unsigned long long)a.count[last]);
      r.sum = a.sum ? (long long)(a.sum_before[last] - a.sum_before[first] + a.sum[last]) : 0LL;
      a.regions[a.kept_off[blockIdx.x] + base + rank] = r;
    }
  }
  if (!WRITE && threadIdx.x == 0) a.chunk_kept[blockIdx.x] = kept;
}

// a count as an operand of the 64-bit scan
struct CountAsU64 {
  __host__ __device__ unsigned long long operator()(int32_t c) const { return (unsigned long long)(long long)c; }
};

}  // namespace fa
