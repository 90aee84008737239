// fa_table.hip.h -- an all-vs-all hit table over ONE genome set reduced on the device: rows -> unordered pairs with their
// symmetric identity -> edges at a cut-off -> connected components (fa_table_pairs / fa_table_clusters).  Nothing here is on
// the mapping path: the kernels run only under those two entry points, on a stream of the call's own.
//
// Semantics (genomes are numbered 0 .. n-1; query_id and ref_genome_id index the same list)
//   1. Filter.  A row (q, r) with q == r never forms a pair.  Another row survives iff
//        (float)((uint64)count_seq * fragment_length) >= (float)min(query_length[q], reference_length[r]) * min_fraction
//      in float32: the test of Mapper._hit_order (_fastani.pyx) and of outputs.filter_rows.  An id outside [0, n), or the same
//      (q, r) in two rows of the table -- surviving or not --, is FA_ERR_INVALID and nothing is returned.
//   2. Pair (a, b), a < b.  identity_ab is the identity of the surviving row with query a and reference b, identity_ba of the
//      one with query b and reference a; a missing direction is NaN (0x7fc00000).  identity is the float64 mean of the two
//      when both survive, else the one that does: bit for bit the cell [a, b] of
//      outputs.identity_matrix(outputs.filter_rows(...), n, n, symmetric=True).  Pairs come out sorted by (a, b).
//   3. Edge.  A pair is an edge iff identity >= (double)min_identity and, with reciprocal != 0, both directions survive.
//   4. Clusters are the connected components of the edges: labels[g] = the smallest genome number of g's component (a genome
//      without an edge labels itself), n_clusters = the number of g with labels[g] == g.
//
// Road.  k_table_keys packs every row into a 64-bit key  a << 33 | b << 2 | direction << 1 | dropped  (direction 1: the
// row's query is b; dropped: q == r or the filter failed; all ones: an id out of range, which also raises the flag).  A radix
// sort of (key, row number) puts the at most two rows of a pair next to each other, direction 0 first, so everything a
// row needs to know is in its two neighbours: equal keys but for the last bit = a duplicate; a surviving row whose
// predecessor is not the surviving other direction = the head of a pair.  Heads (or, for the clusters, heads that are edges)
// are compacted in order by count / scan / write over chunks of one wave's TAB_CHUNK consecutive rows, a head's place inside its
// chunk being the population count of the ballots below its lane (the form of k_map_count / k_chunk_scan / k_map_write;
// the scan is the one kernel of fa_compact.hip.h).
// The same input therefore gives the same bytes on every run: no record's place depends on timing.  (A third form of the
// write kernel keeps an edge's identity, TableEdge: what fa_represent.hip.h selects representatives from.  A fourth takes
// every pair that is present -- no cut-off, `reciprocal` applied -- as the two directed entries (a -> b, b -> a) with its
// fixed-point weight: what fa_linkage.hip.h agglomerates; its count kernel also refuses an identity that has no weight.)
//
// Components run as rounds of two launches.  k_comp_edges lowers, for every edge whose ends carry different labels, the
// larger label's own entry and the entry of the genome that carried it to the smaller label (atomicMin); k_comp_jump
// replaces every label by the root of its chain (labels[g] = labels[labels[g]] to a fixed point).  Every label is at all
// times a genome of its own component and labels only decrease, so any interleaving -- and any stale read, which returns
// an earlier, larger label of the same component -- leaves the invariant intact and can only cost a round.  Every
// cross-workgroup effect is an agent-scope atomicMin / atomicMax / atomicAdd / atomicOr, whose outcome does not depend
// on order.  A round that lowered nothing wrote nothing, so all its reads were current: every edge joins equal labels and
// every label is a root, which is the answer.  The host reads the 4-byte `changed` epoch once per round.
// What a kernel reports to the host -- a flag, the epoch of a round, a count -- it reports once per wave, through wave_flag,
// wave_epoch and wave_count below; the kernels of fa_represent.hip.h, fa_linkage.hip.h and fa_medoid.hip.h use the same three.
#pragma once

#include "fa_common.h"
#include "fa_compact.hip.h"
#include "fa_link.h"

namespace fa {

constexpr int TAB_ITERS = 8, TAB_CHUNK = 64 * TAB_ITERS;          // rows per wave; a workgroup of four waves takes 4 * TAB_CHUNK
constexpr unsigned TAB_BAD_ID = 1u, TAB_DUPLICATE = 2u;
constexpr unsigned TAB_BAD_IDENTITY = 64u;      // (TAB_EMIT_LINK) a present pair whose identity is NaN or outside [0, 128]
constexpr unsigned long long TAB_KEY_NONE = ~0ULL;

// ---- one report per wave ---------------------------------------------------------------------------------------------
// What a kernel of the reductions tells the host goes through one of these three, each CALLED BY EVERY LANE OF THE WAVE (they
// ballot): a wave with something to report issues one atomic, whose result does not depend on the order of the operands.
__device__ __forceinline__ void wave_flag(unsigned int *flags, bool raise, unsigned int flag) {      // *flags |= flag, if any lane says so
  const unsigned long long m = __ballot(raise);
  if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicOr(flags, flag);
}
__device__ __forceinline__ void wave_epoch(unsigned int *epoch, bool report, unsigned int round) {   // *epoch = the last round a lane reports
  const unsigned long long m = __ballot(report);
  if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicMax(epoch, round);
}
__device__ __forceinline__ void wave_count(unsigned int *count, bool counted) {                      // *count += the lanes that say so
  const unsigned long long m = __ballot(counted);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(count, (unsigned int)__popcll(m));
}

// one per call, zeroed before the first launch
struct TableStatus {
  unsigned long long survivors, pairs, edges;   // k_table_count
  int64_t emitted;                              // k_chunk_scan: records the write kernel produces
  unsigned int flags;                           // TAB_BAD_ID | TAB_DUPLICATE
  unsigned int changed;                         // the last round (1-based) in which a label was lowered
  unsigned int roots;                           // k_comp_roots
  unsigned int pad;
};

// an edge with the symmetric identity it passed the cut-off with (the third form k_table_write emits: fa_represent.hip.h)
struct TableEdge {
  int32_t a, b;
  double identity;                     // >= 0; -0.0 is stored as +0.0
};

constexpr int32_t TAB_EMIT_PAIRS = 0, TAB_EMIT_EDGES = 1, TAB_EMIT_WEIGHTED = 2, TAB_EMIT_LINK = 3;

struct TableArgs {
  const fa_cgi_row *rows;
  int64_t n_rows;
  int32_t n_genomes;
  const uint64_t *query_length, *reference_length;
  unsigned long long fragment_length;
  float min_fraction;
  int32_t reciprocal;
  double min_identity;
  const unsigned long long *keys;      // sorted
  const uint32_t *row_of;              // row number of every sorted key
  int32_t n_chunks;
  int32_t emit;                        // TAB_EMIT_*: the pairs as records, the edges as (a, b), the edges as (a, b, identity),
                                       // the present pairs as directed entries
  int32_t link_bits;                   // (TAB_EMIT_LINK) a directed entry's key is from << link_bits | to
  int32_t *chunk_count;                // [n_chunks]
  int64_t *chunk_off;                  // [n_chunks]
  fa_pair *pairs;
  int2 *edges;
  TableEdge *weighted;
  unsigned long long *link_keys;       // [2 * cap]
  LinkSum *link_sums;                  // [2 * cap]
  int64_t cap;                         // room behind `pairs` / `edges` / `weighted`; half of that behind link_keys / link_sums
  TableStatus *status;
};

__global__ __launch_bounds__(256) void k_table_keys(TableArgs a, unsigned long long *keys, uint32_t *row_of) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_rows) return;
  const int32_t q = a.rows[i].query_id, r = a.rows[i].ref_genome_id, count = a.rows[i].count_seq;
  unsigned long long key = TAB_KEY_NONE;
  if ((uint32_t)q >= (uint32_t)a.n_genomes || (uint32_t)r >= (uint32_t)a.n_genomes) atomicOr(&a.status->flags, TAB_BAD_ID);
  else {
    const unsigned long long shared_length = (unsigned long long)(long long)count * a.fragment_length;
    const unsigned long long min_length = min((unsigned long long)a.query_length[q], (unsigned long long)a.reference_length[r]);
    const bool keep = q != r && (float)shared_length >= (float)min_length * a.min_fraction;
    const unsigned long long lo = (unsigned long long)min(q, r), hi = (unsigned long long)max(q, r);
    key = lo << 33 | hi << 2 | (q > r ? 2ULL : 0ULL) | (keep ? 0ULL : 1ULL);
  }
  keys[i] = key;
  row_of[i] = (uint32_t)i;
}

struct TableItem {
  bool survives, duplicate, head, edge;
  int32_t a, b;
  float ab, ba;
  double identity;
};

__device__ __forceinline__ bool table_same_pair(unsigned long long x, unsigned long long y) { return ((x ^ y) >> 2) == 0; }

// what sorted row i is, from its key and its neighbours'; all false beyond the table
__device__ __forceinline__ TableItem table_item(const TableArgs &a, int64_t i) {
  TableItem t;
  t.survives = t.duplicate = t.head = t.edge = false;
  t.a = t.b = 0; t.ab = t.ba = 0.0f; t.identity = 0.0;
  if (i >= a.n_rows) return t;
  const unsigned long long key = a.keys[i];
  const unsigned long long prev = i > 0 ? a.keys[i - 1] : TAB_KEY_NONE;
  t.survives = (key & 1ULL) == 0;
  t.duplicate = i > 0 && (prev >> 1) == (key >> 1);
  t.head = t.survives && !(i > 0 && table_same_pair(prev, key) && (prev & 1ULL) == 0);
  if (!t.head) return t;
  const float nan32 = __uint_as_float(0x7fc00000u);
  const float own = a.rows[a.row_of[i]].identity;
  t.a = (int32_t)(key >> 33);
  t.b = (int32_t)((key >> 2) & 0x7FFFFFFFULL);
  bool both = false;
  if (key & 2ULL) { t.ab = nan32; t.ba = own; }
  else {
    t.ab = own; t.ba = nan32;
    if (i + 1 < a.n_rows) {
      const unsigned long long next = a.keys[i + 1];
      if (table_same_pair(key, next) && (next & 1ULL) == 0) { t.ba = a.rows[a.row_of[i + 1]].identity; both = true; }
    }
  }
  t.identity = both ? ((double)t.ab + (double)t.ba) / 2.0 : (double)own;
  // (TAB_EMIT_LINK: a pair is present whatever its identity)
  t.edge = (a.emit == TAB_EMIT_LINK || t.identity >= a.min_identity) && (both || a.reciprocal == 0);
  return t;
}

__global__ __launch_bounds__(256) void k_table_count(TableArgs a) {
  const int lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= a.n_chunks) return;                                  // (wave-uniform)
  const int64_t base = (int64_t)chunk * TAB_CHUNK + lane;
  int survivors = 0, pairs = 0, edges = 0;
  bool duplicate = false, bad_identity = false;
#pragma unroll
  for (int u = 0; u < TAB_ITERS; u++) {
    const TableItem t = table_item(a, base + 64 * u);
    survivors += __popcll(__ballot(t.survives));
    pairs += __popcll(__ballot(t.head));
    edges += __popcll(__ballot(t.edge));
    duplicate |= t.duplicate;
    bad_identity |= a.emit == TAB_EMIT_LINK && t.edge && !link_identity_ok(t.identity);
  }
  if (__any(duplicate) && lane == 0) atomicOr(&a.status->flags, TAB_DUPLICATE);
  if (__any(bad_identity) && lane == 0) atomicOr(&a.status->flags, TAB_BAD_IDENTITY);
  if (lane != 0) return;
  a.chunk_count[chunk] = a.emit != TAB_EMIT_PAIRS ? edges : pairs;
  if (survivors) atomicAdd(&a.status->survivors, (unsigned long long)survivors);
  if (pairs) atomicAdd(&a.status->pairs, (unsigned long long)pairs);
  if (edges) atomicAdd(&a.status->edges, (unsigned long long)edges);
}

__global__ __launch_bounds__(256) void k_table_write(TableArgs a) {
  const int lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= a.n_chunks || a.chunk_count[chunk] == 0) return;    // (wave-uniform)
  const int64_t base = (int64_t)chunk * TAB_CHUNK + lane;
  int64_t off = a.chunk_off[chunk];
  const unsigned long long below = (1ULL << lane) - 1ULL;
#pragma unroll
  for (int u = 0; u < TAB_ITERS; u++) {
    const TableItem t = table_item(a, base + 64 * u);
    const bool emit = a.emit != TAB_EMIT_PAIRS ? t.edge : t.head;
    const unsigned long long mask = __ballot(emit);
    const int64_t o = off + __popcll(mask & below);
    off += __popcll(mask);
    if (!emit || o >= a.cap) continue;
    if (a.emit == TAB_EMIT_LINK) {
      const LinkSum one{link_fixed(t.identity), 1};
      a.link_keys[2 * o] = (unsigned long long)t.a << a.link_bits | (unsigned long long)t.b;
      a.link_keys[2 * o + 1] = (unsigned long long)t.b << a.link_bits | (unsigned long long)t.a;
      a.link_sums[2 * o] = one;
      a.link_sums[2 * o + 1] = one;
    } else if (a.emit == TAB_EMIT_WEIGHTED) {
      TableEdge e;
      e.a = t.a; e.b = t.b; e.identity = t.identity == 0.0 ? 0.0 : t.identity;
      a.weighted[o] = e;
    } else if (a.emit == TAB_EMIT_EDGES) a.edges[o] = make_int2(t.a, t.b);
    else {
      fa_pair p;
      p.a = t.a; p.b = t.b; p.identity_ab = t.ab; p.identity_ba = t.ba; p.identity = t.identity;
      a.pairs[o] = p;
    }
  }
}

// ---- connected components ------------------------------------------------------------------------------------------
struct CompArgs {
  const int2 *edges;
  int64_t n_edges;
  int32_t *labels;
  int32_t n_genomes;
  unsigned int round;                  // 1-based
  TableStatus *status;
};

__global__ __launch_bounds__(256) void k_comp_init(int32_t *labels, int32_t n) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g < n) labels[g] = (int32_t)g;
}

// a label as the memory side holds it where the hardware allows (fewer rounds); correctness does not rest on it
__device__ __forceinline__ int32_t comp_label(const int32_t *labels, int32_t g) {
  return __hip_atomic_load(labels + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}


__global__ __launch_bounds__(256) void k_comp_edges(CompArgs c) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool lowered = false;
  if (i < c.n_edges) {
    const int2 e = c.edges[i];
    const int32_t la = comp_label(c.labels, e.x), lb = comp_label(c.labels, e.y);
    if (la != lb) {
      const int32_t lo = min(la, lb), hi = max(la, lb), carrier = la > lb ? e.x : e.y;
      lowered = atomicMin(c.labels + hi, lo) > lo;
      lowered |= atomicMin(c.labels + carrier, lo) > lo;
    }
  }
  wave_epoch(&c.status->changed, lowered, c.round);
}

__global__ __launch_bounds__(256) void k_comp_jump(CompArgs c) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool lowered = false;
  if (g < c.n_genomes) {
    const int32_t first = comp_label(c.labels, (int32_t)g);
    int32_t l = first;
    for (;;) {                                                   // (a chain descends strictly: it ends at a root)
      const int32_t up = comp_label(c.labels, l);
      if (up >= l) break;
      l = up;
    }
    if (l < first) lowered = atomicMin(c.labels + g, l) > l;
  }
  wave_epoch(&c.status->changed, lowered, c.round);
}

// the genomes that label themselves, added to *roots (of any labels, not only those of the components)
__global__ __launch_bounds__(256) void k_comp_roots(const int32_t *labels, int32_t n, unsigned int *roots) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  wave_count(roots, g < n && labels[g] == (int32_t)g);
}

}  // namespace fa
