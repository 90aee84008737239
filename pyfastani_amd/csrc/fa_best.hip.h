// fa_best.hip.h -- a query x reference hit table reduced on the device to every query's k best hits (fa_table_best): the
// closest references that pass an identity and an aligned-fraction cut-off, classification's counterpart of the pairs and
// clusters of fa_table.hip.h.  Nothing here is on the mapping path: the kernels run only under that entry point, on a
// stream of the call's own.
//
// Semantics (queries are numbered 0 .. n_queries-1, references 0 .. n_references-1; the two lists are unrelated)
//   1. Survival.  A row (q, r) survives iff all four hold, each evaluated in float32 exactly as written:
//        self rows         not (exclude_self and q == r)
//        minimum fraction  (float)((uint64)count_seq * fragment_length) >= (float)min(query_length[q], reference_length[r]) * min_fraction
//                          -- the test of Mapper._hit_order (_fastani.pyx) and of outputs.filter_rows
//        identity          the sign bit of identity is clear, it is not NaN, and identity >= min_identity
//        aligned fraction  (float)count_seq >= (float)total_query_fragments * min_aligned_fraction
//      An id outside its range, or the same (q, r) in two rows of the table -- surviving or not --, is FA_ERR_INVALID and
//      nothing is returned.
//   2. Order.  The survivors of a query are ordered by identity descending, ties by ref_genome_id ascending: with k >= the
//      number of survivors the order of the Hit list query_draft returns (a stable sort by decreasing identity over rows in
//      reference order).  Survivors have non-negative identities, so the order of the bit patterns is the order of the values.
//   3. Output.  best holds the first min(k, survivors) rows of every query, queries ascending, a query's rows in rank
//      order, every record the 20 bytes of its input row; offsets [n_queries + 1] delimits the queries' records.
//
// Road.  k_best_keys packs every row into  q << ref_bits | r  (ref_bits: those of the largest reference number; all ones: an
// id out of range, which also raises the flag).  A stable radix sort of (key, row number) puts every query's rows
// together in reference order; equal neighbours are duplicates.  k_best_rank_keys walks the sorted rows, applies the four
// tests and gives a survivor  q << 32 | (0xFFFFFFFF - identity bits), every other row all ones.  A second stable radix sort
// puts a query's survivors in rank order -- stability is what keeps ref_genome_id ascending inside equal identities -- and
// every other row behind the last query.  k_best_segments writes, for every query with survivors, where its segment starts and
// ends (the one thread that sees the boundary writes it: no atomics); k_best_scan takes the exclusive 64-bit sum of
// min(k, survivors) over the queries -- the offsets -- and the three counters; k_best_write copies sorted row i to
// best[offsets[q] + (i - start[q])] when that rank is below k.  Every record's place is a function of the two sorted orders,
// and the sorts are stable: the same input gives the same bytes on every run, no record's place depends on timing.
#pragma once

#include "fa_table.hip.h"

namespace fa {

// one per call, zeroed before the first launch
struct BestStatus {
  long long survivors, queries, records;        // k_best_scan
  unsigned int flags;                           // TAB_BAD_ID | TAB_DUPLICATE
  unsigned int pad;
};

struct BestArgs {
  const fa_cgi_row *rows;
  int64_t n_rows;
  int32_t n_queries, n_references;
  const uint64_t *query_length, *reference_length;
  unsigned long long fragment_length;
  float min_fraction, min_identity, min_aligned_fraction;
  int32_t k, exclude_self;
  uint32_t ref_bits;                   // bits of r in the first key
  const unsigned long long *keys;      // sorted: the first keys for k_best_rank_keys, the rank keys after it
  const uint32_t *row_of;              // row number of every sorted key
  int32_t *seg_start, *seg_end;        // [n_queries], zeroed: sorted positions [start, end) of every query's survivors
  int64_t *offsets;                    // [n_queries + 1]
  int32_t *best;                       // five words per record
  BestStatus *status;
};

__global__ __launch_bounds__(256) void k_best_keys(BestArgs a, unsigned long long *keys, uint32_t *row_of) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_rows) return;
  const int32_t q = a.rows[i].query_id, r = a.rows[i].ref_genome_id;
  unsigned long long key = TAB_KEY_NONE;
  if ((uint32_t)q >= (uint32_t)a.n_queries || (uint32_t)r >= (uint32_t)a.n_references) atomicOr(&a.status->flags, TAB_BAD_ID);
  else key = (unsigned long long)q << a.ref_bits | (unsigned long long)r;
  keys[i] = key;
  row_of[i] = (uint32_t)i;
}

// over the rows sorted by (q, r): duplicates, and the key of the second sort; `row_of` keeps its order
__global__ __launch_bounds__(256) void k_best_rank_keys(BestArgs a, unsigned long long *rank_keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_rows) return;
  const unsigned long long key = a.keys[i];
  unsigned long long rank_key = TAB_KEY_NONE;
  if (key != TAB_KEY_NONE) {                                        // (an id out of range: the call fails, the row is skipped)
    if (i > 0 && a.keys[i - 1] == key) atomicOr(&a.status->flags, TAB_DUPLICATE);
    const fa_cgi_row row = a.rows[a.row_of[i]];
    const int32_t q = row.query_id, r = row.ref_genome_id;
    const unsigned long long shared_length = (unsigned long long)(long long)row.count_seq * a.fragment_length;
    const unsigned long long min_length = min((unsigned long long)a.query_length[q], (unsigned long long)a.reference_length[r]);
    const uint32_t bits = __float_as_uint(row.identity);
    bool keep = !(a.exclude_self && q == r);
    keep = keep && (float)shared_length >= (float)min_length * a.min_fraction;
    keep = keep && (bits >> 31) == 0 && row.identity >= a.min_identity;                  // (a NaN compares false)
    keep = keep && (float)row.count_seq >= (float)row.total_query_fragments * a.min_aligned_fraction;
    if (keep) rank_key = (unsigned long long)q << 32 | (unsigned long long)(0xFFFFFFFFu - bits);
  }
  rank_keys[i] = rank_key;
}

// over the rows sorted by rank key: the ends of every query's run of survivors
__global__ __launch_bounds__(256) void k_best_segments(BestArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_rows) return;
  const unsigned long long key = a.keys[i];
  if (key == TAB_KEY_NONE) return;
  const uint32_t q = (uint32_t)(key >> 32);
  if (i == 0 || (uint32_t)(a.keys[i - 1] >> 32) != q) a.seg_start[q] = (int32_t)i;
  if (i + 1 == a.n_rows || a.keys[i + 1] == TAB_KEY_NONE || (uint32_t)(a.keys[i + 1] >> 32) != q) a.seg_end[q] = (int32_t)(i + 1);
}

// exclusive 64-bit sum of min(k, survivors) over the queries by one workgroup (thread t owns a run of consecutive queries, the
// form of k_chunk_scan, fa_compact.hip.h) + the total behind it + the counters
__global__ __launch_bounds__(1024) void k_best_scan(BestArgs a) {
  __shared__ long long sh_wave[16], sh_survivors[16], sh_queries[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t per = ((int64_t)a.n_queries + 1023) / 1024;
  const int64_t c0 = min((int64_t)a.n_queries, (int64_t)threadIdx.x * per), c1 = min((int64_t)a.n_queries, c0 + per);
  long long mine = 0, survivors = 0, queries = 0;
  for (int64_t c = c0; c < c1; c++) {
    const int32_t count = a.seg_end[c] - a.seg_start[c];
    mine += min(count, a.k);
    survivors += count;
    queries += count > 0 ? 1 : 0;
  }
  long long incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long v = __shfl_up(incl, d);
    if (lane >= d) incl += v;
    survivors += __shfl_xor(survivors, d);
    queries += __shfl_xor(queries, d);
  }
  if (lane == 63) { sh_wave[wv] = incl; sh_survivors[wv] = survivors; sh_queries[wv] = queries; }
  __syncthreads();
  long long off = incl - mine;
  for (int w = 0; w < wv; w++) off += sh_wave[w];
  for (int64_t c = c0; c < c1; c++) { a.offsets[c] = off; off += min(a.seg_end[c] - a.seg_start[c], a.k); }
  if (threadIdx.x == 1023) {
    long long s = 0, n = 0;
    for (int w = 0; w < 16; w++) { s += sh_survivors[w]; n += sh_queries[w]; }
    a.offsets[a.n_queries] = off;
    a.status->records = off; a.status->survivors = s; a.status->queries = n;
  }
}

__global__ __launch_bounds__(256) void k_best_write(BestArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_rows) return;
  const unsigned long long key = a.keys[i];
  if (key == TAB_KEY_NONE) return;
  const uint32_t q = (uint32_t)(key >> 32);
  const int64_t rank = i - a.seg_start[q];
  if (rank >= a.k) return;
  const int32_t *src = reinterpret_cast<const int32_t *>(a.rows + a.row_of[i]);
  int32_t *dst = a.best + (a.offsets[q] + rank) * 5;
#pragma unroll
  for (int w = 0; w < 5; w++) dst[w] = src[w];
}

}  // namespace fa
