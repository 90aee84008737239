// fa_represent.hip.h -- greedy representative clustering of an all-vs-all hit table on the device (fa_table_representatives):
// rows -> edges with their symmetric identity -> the representatives in the caller's order of preference -> every other
// genome's closest representative.  Nothing here is on the mapping path: the kernels run only under that entry point, on a
// stream of the call's own.
//
// Semantics (genomes are numbered 0 .. n-1; query_id and ref_genome_id index the same list)
//   1. Filter, pair, edge: steps 1-3 of fa_table.hip.h, `reciprocal` included.  min_identity is a number >= 0, so every
//      edge's identity is >= 0; -0.0 counts and is returned as +0.0.
//   2. Order.  order [n] is a permutation of the genome numbers, the most preferred first (null: genome-number order);
//      pos[g] is the place of g in it (fa_order.h).
//   3. Representatives.  Walking the genomes in `order`, a genome is a representative iff it has no edge to a representative
//      of smaller pos: R is the one set with  g in R  <=>  no neighbour h with pos[h] < pos[g] is in R  (the
//      lexicographically first maximal independent set of the edges under `order`).
//   4. Assignment.  labels[g] = g and identity[g] = 100.0 for a representative.  Any other genome has a neighbour in R; it
//      gets the one of largest symmetric identity compared as float64, ties to the smaller pos, and that identity.
//      n_representatives = the number of g with labels[g] == g.
//
// Road.  The front end is that of fa_table.hip.h (keys, radix sort, count / scan / write); k_table_write emits its third
// form, TableEdge (a, b, identity), in (a, b) order.
//
// Selection runs as rounds of two launches over state[g] in {undecided, representative, member}.  k_rep_edges looks at every
// edge (u, v), pos[u] < pos[v], whose v is undecided: a representative u makes v a member; an undecided u marks v held back
// in this round (blocked[v] = round).  k_rep_decide then turns every genome that is still undecided and was not held back
// in this round into a representative.  A decision is only ever made when it is final:
//   - `member` is written only beside a neighbour read as `representative`, and `representative` is written only by
//     k_rep_decide, in an earlier launch: that read cannot be wrong, and a genome next to an earlier representative is a
//     member by definition.
//   - `representative` is written only to a genome none of whose earlier neighbours was read as representative (it would be
//     a member) or as undecided (it would be held back): all of them were read as members, which is final, so none is in R.
//   A stale read inside k_rep_edges can only return `undecided` for a genome that has just become a member: it holds a
//   genome back for a round and changes no decision.  Every cross-workgroup effect is an agent-scope atomicMax / atomicMin /
//   atomicAdd / atomicOr, whose outcome does not depend on order.
// The undecided genome of smallest pos has only decided earlier neighbours: a round makes it a member or a representative.
// So every round decides at least one genome and the loop ends within n rounds (a path walked in its own order needs about
// that many); the host caps it there.  It reads the 4-byte `changed` epoch once per round: the last round after which a genome
// was still undecided (wave_epoch; the representatives are counted with wave_count: fa_table.hip.h has both).
//
// Assignment is two passes over the edges with one end a representative and the other a member: an atomicMax of the identity's
// bit pattern per member (non-negative doubles order like their bits), then an atomicMin of the representative's pos over the
// edges that attain it.  k_rep_write turns (state, best, nearest) into labels and identities.  No value depends on timing,
// so the same input gives the same bytes on every run.
#pragma once

#include "fa_table.hip.h"

namespace fa {

constexpr int32_t REP_UNDECIDED = 0, REP_CHOSEN = 1, REP_MEMBER = 2;
constexpr unsigned TAB_NO_NEAREST = 4u;        // (TableStatus::flags) a member without a representative neighbour: never

struct RepArgs {
  const TableEdge *edges;
  int64_t n_edges;
  int32_t n_genomes;
  const int32_t *pos;                  // [n] the place of every genome in the order
  const int32_t *order;                // [n] its inverse
  int32_t *state;                      // [n] REP_*
  unsigned int *blocked;               // [n] the last round in which an undecided earlier neighbour held the genome back
  unsigned long long *best;            // [n] the bits of the largest identity among a member's representative neighbours
  int32_t *nearest;                    // [n] the smallest pos among those that attain it
  int32_t *labels;
  double *identity;                    // may be null
  unsigned int round;                  // 1-based
  TableStatus *status;
};

__global__ __launch_bounds__(256) void k_rep_init(RepArgs r, int32_t state) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= r.n_genomes) return;
  r.state[g] = state;
  r.blocked[g] = 0u;
  r.best[g] = 0ULL;
  r.nearest[g] = INT32_MAX;
}

// a state as the memory side holds it where the hardware allows (fewer rounds); correctness does not rest on it
__device__ __forceinline__ int32_t rep_state(const int32_t *state, int32_t g) {
  return __hip_atomic_load(state + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_rep_edges(RepArgs r) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= r.n_edges) return;
  const TableEdge e = r.edges[i];
  const bool a_first = r.pos[e.a] < r.pos[e.b];
  const int32_t u = a_first ? e.a : e.b, v = a_first ? e.b : e.a;
  if (rep_state(r.state, v) != REP_UNDECIDED) return;
  const int32_t su = rep_state(r.state, u);
  if (su == REP_CHOSEN) atomicMax(r.state + v, REP_MEMBER);
  else if (su == REP_UNDECIDED) atomicMax(r.blocked + v, r.round);
}

__global__ __launch_bounds__(256) void k_rep_decide(RepArgs r) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool pending = false;
  if (g < r.n_genomes && r.state[g] == REP_UNDECIDED) {
    if (r.blocked[g] != r.round) r.state[g] = REP_CHOSEN;
    else pending = true;
  }
  wave_epoch(&r.status->changed, pending, r.round);                // the last round that leaves a genome undecided
}

// the member and the representative of an edge that joins one of each (the only edges the assignment looks at)
__device__ __forceinline__ bool rep_member_edge(const RepArgs &r, const TableEdge &e, int32_t &member, int32_t &chosen) {
  const int32_t sa = r.state[e.a], sb = r.state[e.b];
  if (sa == REP_MEMBER && sb == REP_CHOSEN) { member = e.a; chosen = e.b; return true; }
  if (sb == REP_MEMBER && sa == REP_CHOSEN) { member = e.b; chosen = e.a; return true; }
  return false;
}

__global__ __launch_bounds__(256) void k_rep_best(RepArgs r) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= r.n_edges) return;
  const TableEdge e = r.edges[i];
  int32_t member, chosen;
  if (rep_member_edge(r, e, member, chosen)) atomicMax(r.best + member, (unsigned long long)__double_as_longlong(e.identity));
}

__global__ __launch_bounds__(256) void k_rep_nearest(RepArgs r) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= r.n_edges) return;
  const TableEdge e = r.edges[i];
  int32_t member, chosen;
  if (rep_member_edge(r, e, member, chosen) && (unsigned long long)__double_as_longlong(e.identity) == r.best[member])
    atomicMin(r.nearest + member, r.pos[chosen]);
}

__global__ __launch_bounds__(256) void k_rep_write(RepArgs r) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool chosen = false;
  if (g < r.n_genomes) {
    chosen = r.state[g] == REP_CHOSEN;
    int32_t label = (int32_t)g;
    if (!chosen) {
      const int32_t at = r.nearest[g];
      if ((uint32_t)at < (uint32_t)r.n_genomes) label = r.order[at];
      else atomicOr(&r.status->flags, TAB_NO_NEAREST);
    }
    r.labels[g] = label;
    if (r.identity) r.identity[g] = chosen ? 100.0 : __longlong_as_double((long long)r.best[g]);
  }
  wave_count(&r.status->roots, chosen);
}

}  // namespace fa
