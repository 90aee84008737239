// fa_reduce.hip.h -- the host drivers of the reductions over results the mapper already holds: a hit table to pairs,
// clusters, representatives, average-linkage clusters and their dendrogram with its cuts, and the medoids of given clusters (fa_table.hip.h, fa_represent.hip.h, fa_linkage.hip.h, fa_medoid.hip.h), to every query's k best hits (fa_best.hip.h), the
// fragment mappings behind a table to a per-fragment conservation profile and its per-genome summary (fa_profile.hip.h), the
// same records to a profile by reference bin and either profile to its regions (fa_refprofile.hip.h), the
// signature screen (fa_screen.hip.h) and its containment road (fa_contain.hip.h).  They use nothing of the sketch, the mapper or the workspace -- but for the last one, the
// signatures of a resident batch (fa_batchsig.hip.h), which borrows a workspace for K1's staging arrays; fa_engine.hip wraps each
// in its extern "C" entry point.
//
// Every driver has the same frame (the pieces are in fa_common.h): it checks its arguments, then require_device(), then
//   - runs on a stream of the call's own (CallStream), declared before every buffer so that it outlives them;
//   - owns a status block (StatusBlock) zeroed on that stream before the first launch, and turns the flags it reads back
//     into the entry point's own error messages;
//   - takes every input as the caller's device pointer or uploads it (on_device), and writes every output to the caller's
//     device pointer or to a staged copy that is downloaded at the end (Staged);
//   - sizes its sort keys with bit_width_u64 / id_bits and calls rocPRIM through with_temp;
//   - is synchronised when it returns: host outputs are complete, device outputs are written.
//
// The six reductions of an all-vs-all table share the first half of that frame as code (check_table_args, TableFront); each
// then has a driver of its own, table_<what>, that reads top to bottom.  What two of them share they share through a function
// (check_linkage_args, linkage, count_roots), never through a flag: a seventh reduction is a seventh driver.
#pragma once

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <climits>
#include <vector>

#include "fa_batch.hip.h"
#include "fa_batchsig.hip.h"
#include "fa_best.hip.h"
#include "fa_common.h"
#include "fa_contain.hip.h"
#include "fa_linkage.hip.h"
#include "fa_medoid.hip.h"
#include "fa_order.h"
#include "fa_profile.hip.h"
#include "fa_query.hip.h"
#include "fa_refprofile.hip.h"
#include "fa_represent.hip.h"
#include "fa_screen.hip.h"
#include "fa_table.hip.h"

namespace fa {

// ------------------------------------------------------------------------------------------------------------
// The hit table of an all-vs-all reduced to pairs and clusters (fa_table.hip.h has the semantics and the road)
// ------------------------------------------------------------------------------------------------------------
// the genomes among n > 0 that label themselves (device labels), counted in the call's zeroed `status`; synchronises the stream
inline unsigned int count_roots(const int32_t *labels, int32_t n, TableStatus *status, hipStream_t st) {
  unsigned int roots = 0;
  hipLaunchKernelGGL(k_comp_roots, dim3(ceil_div(n, 256)), dim3(256), 0, st, labels, n, &status->roots);
  FA_HIP(hipGetLastError());
  FA_HIP(hipMemcpyAsync(&roots, &status->roots, sizeof roots, hipMemcpyDeviceToHost, st));
  FA_HIP(hipStreamSynchronize(st));
  return roots;
}

// The connected components of an edge list over n_genomes > 0 genomes (fa_table.hip.h): labels (device) receive every genome's
// smallest group member; returns the number of groups and, in `rounds`, those of the loop.  `status` is the call's zeroed
// TableStatus; the stream is synchronised on return.
inline unsigned int components(const int2 *edges, int64_t n_edges, int32_t *labels, int32_t n_genomes, TableStatus *status, hipStream_t st,
                               int64_t &rounds) {
  CompArgs c{};
  c.edges = edges; c.n_edges = n_edges; c.labels = labels; c.n_genomes = n_genomes; c.status = status;
  const dim3 genome_grid(ceil_div(n_genomes, 256));
  hipLaunchKernelGGL(k_comp_init, genome_grid, dim3(256), 0, st, c.labels, n_genomes);
  rounds = 0;
  if (n_edges) {
    // a round lowers at least one label or is the last; labels only decrease, so the loop ends (fa_table.hip.h)
    for (;;) {
      c.round = (unsigned int)++rounds;
      hipLaunchKernelGGL(k_comp_edges, dim3(ceil_div(n_edges, 256)), dim3(256), 0, st, c);
      hipLaunchKernelGGL(k_comp_jump, genome_grid, dim3(256), 0, st, c);
      FA_HIP(hipGetLastError());
      unsigned int changed = 0;
      FA_HIP(hipMemcpyAsync(&changed, &status->changed, sizeof changed, hipMemcpyDeviceToHost, st));
      FA_HIP(hipStreamSynchronize(st));
      if (changed != c.round) break;
    }
  }
  return count_roots(labels, n_genomes, status, st);
}

// The representatives of a weighted edge list over n_genomes > 0 genomes and every other genome's closest one
// (fa_represent.hip.h): labels and identity (device, identity may be null) are written once the selection has ended; returns
// the number of representatives and, in `rounds`, those of the selection loop.  `pos` and `order` are device arrays.  `status`
// is the call's zeroed TableStatus; the stream is synchronised on return.
inline unsigned int representatives(const TableEdge *edges, int64_t n_edges, const int32_t *pos, const int32_t *order, int32_t *labels,
                                    double *identity, int32_t n_genomes, TableStatus *status, hipStream_t st, int64_t &rounds) {
  DevBuf<int32_t> words;                      // state, blocked, nearest
  DevBuf<unsigned long long> best;
  words.ensure((size_t)n_genomes * 3);
  best.ensure((size_t)n_genomes);
  RepArgs r{};
  r.edges = edges; r.n_edges = n_edges; r.n_genomes = n_genomes; r.pos = pos; r.order = order;
  r.state = words.p; r.blocked = reinterpret_cast<unsigned int *>(words.p + n_genomes); r.nearest = words.p + 2 * (size_t)n_genomes;
  r.best = best.p; r.labels = labels; r.identity = identity; r.status = status;
  const dim3 genome_grid(ceil_div(n_genomes, 256)), edge_grid(ceil_div(n_edges, 256));
  // without an edge every genome stands for itself
  hipLaunchKernelGGL(k_rep_init, genome_grid, dim3(256), 0, st, r, n_edges ? REP_UNDECIDED : REP_CHOSEN);
  rounds = 0;
  if (n_edges) {
    // a round decides at least the undecided genome of smallest pos, so there are at most n_genomes of them (fa_represent.hip.h)
    for (;;) {
      r.round = (unsigned int)++rounds;
      hipLaunchKernelGGL(k_rep_edges, edge_grid, dim3(256), 0, st, r);
      hipLaunchKernelGGL(k_rep_decide, genome_grid, dim3(256), 0, st, r);
      FA_HIP(hipGetLastError());
      unsigned int pending = 0;
      FA_HIP(hipMemcpyAsync(&pending, &status->changed, sizeof pending, hipMemcpyDeviceToHost, st));
      FA_HIP(hipStreamSynchronize(st));
      if (pending != r.round) break;
      FA_REQUIRE(rounds < (int64_t)n_genomes, FA_ERR_INTERNAL, "the selection of representatives did not end within n_genomes rounds");
    }
    hipLaunchKernelGGL(k_rep_best, edge_grid, dim3(256), 0, st, r);
    hipLaunchKernelGGL(k_rep_nearest, edge_grid, dim3(256), 0, st, r);
  }
  hipLaunchKernelGGL(k_rep_write, genome_grid, dim3(256), 0, st, r);
  FA_HIP(hipGetLastError());
  TableStatus end{};
  FA_HIP(hipMemcpyAsync(&end, status, sizeof end, hipMemcpyDeviceToHost, st));
  FA_HIP(hipStreamSynchronize(st));
  FA_REQUIRE(!(end.flags & TAB_NO_NEAREST), FA_ERR_INTERNAL, "a genome that is no representative has no representative neighbour");
  return end.roots;
}

// the table as all six entry points take it: their first seven arguments
struct TableIn {
  const fa_cgi_row *rows; int64_t n_rows; bool rows_device; int32_t n_genomes; const uint64_t *query_lengths, *reference_lengths; const fa_table_params *p;
};
// the checks the six share; each driver goes on with its own
inline void check_table_args(const TableIn &in) {
  FA_REQUIRE(in.p, FA_ERR_INVALID, "null table parameters");
  FA_REQUIRE(in.p->fragment_length >= 1, FA_ERR_INVALID, "fragment_length must be strictly positive");
  FA_REQUIRE(in.n_genomes >= 0 && in.n_rows >= 0, FA_ERR_INVALID, "negative table size");
  FA_REQUIRE(in.n_rows == 0 || in.rows, FA_ERR_INVALID, "null rows");
  FA_REQUIRE(in.n_genomes == 0 || (in.query_lengths && in.reference_lengths), FA_ERR_INVALID, "null genome lengths");
  FA_REQUIRE(in.n_rows <= (int64_t)INT32_MAX, FA_ERR_UNSUPPORTED, "a table of more than 2^31 - 1 rows");
}

// The front end of the six (fa_table.hip.h): the call's stream and status block, the rows and lengths on the device, the sorted
// keys, and the count and scan of the records of the call's one form (TAB_EMIT_*: k_table_count depends on it).  Constructed,
// the table has passed its device checks -- a refused one throws before a driver has touched an output -- and `status` and
// `n_emit` are read; the driver then has the records written by the emit call of its form.
struct TableFront {
  CallStream stream; hipStream_t st;          // the stream first: it outlives the buffers
  StatusBlock<TableStatus> d_status;          // d_status.p: also the `changed` and `roots` of the loops behind the front end
  TableStatus status{};                       // its host copy after k_chunk_scan (all zero for a table without rows)
  int64_t n_emit = 0;                         // records of the call's form
  DevBuf<unsigned char> temp;                 // rocPRIM's; free for the driver's own sorts afterwards

  TableFront(const TableIn &in, int32_t emit) : st(stream.s), d_status(st) {
    const int64_t n_rows = in.n_rows; const int32_t n_genomes = in.n_genomes;
    a.n_rows = n_rows; a.n_genomes = n_genomes;
    a.fragment_length = (unsigned long long)in.p->fragment_length; a.min_fraction = in.p->min_fraction;
    a.min_identity = (double)in.p->min_identity; a.reciprocal = in.p->reciprocal;
    a.emit = emit; a.link_bits = (int32_t)id_bits(n_genomes); a.status = d_status.p;
    a.n_chunks = ceil_div(n_rows, TAB_CHUNK);
    if (!n_rows) return;
    a.rows = on_device(in.rows, in.rows_device, (size_t)n_rows, d_rows, st);
    d_len.ensure((size_t)n_genomes * 2);
    FA_HIP(hipMemcpyAsync(d_len.p, in.query_lengths, (size_t)n_genomes * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    FA_HIP(hipMemcpyAsync(d_len.p + n_genomes, in.reference_lengths, (size_t)n_genomes * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    a.query_length = d_len.p; a.reference_length = d_len.p + n_genomes;
    keys.ensure((size_t)n_rows); keys_sorted.ensure((size_t)n_rows);
    row_of.ensure((size_t)n_rows); row_of_sorted.ensure((size_t)n_rows);
    hipLaunchKernelGGL(k_table_keys, dim3(ceil_div(n_rows, 256)), dim3(256), 0, st, a, keys.p, row_of.p);
    // the bits a key of this table can have set: two flag bits, 31 of b, and those of the largest a
    const unsigned end_bit = 33u + id_bits(n_genomes);
    with_temp(temp, [&](void *t, size_t &bytes) {
      return rocprim::radix_sort_pairs(t, bytes, keys.p, keys_sorted.p, row_of.p, row_of_sorted.p, (size_t)n_rows, 0u, end_bit, st);
    });
    a.keys = keys_sorted.p; a.row_of = row_of_sorted.p;
    chunk_count.ensure((size_t)a.n_chunks); chunk_off.ensure((size_t)a.n_chunks);
    a.chunk_count = chunk_count.p; a.chunk_off = chunk_off.p;
    hipLaunchKernelGGL(k_table_count, dim3(ceil_div(a.n_chunks, 4)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_chunk_scan, dim3(1), dim3(1024), 0, st, a.chunk_count, a.chunk_off, a.n_chunks, &d_status.p->emitted);
    FA_HIP(hipGetLastError());
    status = d_status.read(st);
    FA_REQUIRE(!(status.flags & TAB_BAD_ID), FA_ERR_INVALID, "a row names a genome outside [0, n_genomes)");
    FA_REQUIRE(!(status.flags & TAB_DUPLICATE), FA_ERR_INVALID, "the table holds the same (query, reference) twice");
    FA_REQUIRE(!(status.flags & TAB_BAD_IDENTITY), FA_ERR_INVALID, "a present pair has an identity that is NaN or outside [0, 128]");
    n_emit = (int64_t)status.emitted;
  }
  // the n_emit records into room for as many (link: for 2 * n_emit directed entries); nothing is launched for none
  void emit_pairs(fa_pair *pairs) { a.pairs = pairs; emit(TAB_EMIT_PAIRS); }
  void emit_edges(int2 *edges) { a.edges = edges; emit(TAB_EMIT_EDGES); }
  void emit_weighted(TableEdge *edges) { a.weighted = edges; emit(TAB_EMIT_WEIGHTED); }
  void emit_link(unsigned long long *link_keys, LinkSum *link_sums) { a.link_keys = link_keys; a.link_sums = link_sums; emit(TAB_EMIT_LINK); }
  // slots 0-3 of an entry point's stats (null: none): survivors, pairs, edges, and the entry point's own fourth
  void write_stats(int64_t *stats, int64_t fourth) const {
    if (stats) { stats[0] = (int64_t)status.survivors; stats[1] = (int64_t)status.pairs; stats[2] = (int64_t)status.edges; stats[3] = fourth; }
  }

 private:
  DevBuf<fa_cgi_row> d_rows; DevBuf<uint64_t> d_len;
  DevBuf<unsigned long long> keys, keys_sorted;
  DevBuf<uint32_t> row_of, row_of_sorted;
  DevBuf<int32_t> chunk_count; DevBuf<int64_t> chunk_off;
  TableArgs a{};
  void emit(int32_t form) {
    FA_REQUIRE(form == a.emit, FA_ERR_INTERNAL, "the front end of a table counted another form than the one asked for");
    if (!n_emit) return;
    a.cap = n_emit;
    hipLaunchKernelGGL(k_table_write, dim3(ceil_div(a.n_chunks, 4)), dim3(256), 0, st, a);
  }
};

// `missing` and `min_identity` of fa_table_linkage and fa_table_dendrogram, checked and in fixed point (fa_link.h)
struct LinkCutoffs { long long qm, qc; };
inline LinkCutoffs check_linkage_args(const fa_table_params *p, float missing, int32_t n_genomes) {
  FA_REQUIRE(p->min_identity >= 0.0f, FA_ERR_INVALID, "min_identity must be a number that is not negative");          // (false for NaN)
  FA_REQUIRE(missing >= 0.0f, FA_ERR_INVALID, "missing must be a number that is not negative");
  const double dm = rint((double)missing * LINK_SCALE), dc = rint((double)p->min_identity * LINK_SCALE);
  FA_REQUIRE(dm < dc, FA_ERR_INVALID, "missing must lie below min_identity");
  FA_REQUIRE(n_genomes <= LINK_MAX_GENOMES, FA_ERR_UNSUPPORTED, "average linkage over more than 2^18 genomes");
  // no weight exceeds LINK_MAX_W: a cut-off above it merges nothing whatever its value, and neither does the clamped one
  // (link_cutoff of fa_link.h is this rule for one float: fa_dendrogram_cut forms its qc with it, and clusters._fixed_cutoff
  // restates it in Python; the three must stay one rule for a cut to give the bytes of this call)
  return {(long long)std::min(dm, (double)LINK_MAX_W), (long long)std::min(dc, (double)(LINK_MAX_W + 1))};
}

// The average-linkage clusters of the present pairs of a table over n_genomes > 0 genomes (fa_linkage.hip.h): labels (device)
// receive every genome's smallest cluster member; returns the number of clusters and, in `rounds`, the rounds that merged a
// pair.  The front end's form is TAB_EMIT_LINK; its stream is synchronised on return.  With `merges` (device, room for
// n_genomes - 1: fa_table_dendrogram) every merge is recorded there, in no order, and *n_merges is their number.
inline unsigned int linkage(TableFront &front, int32_t *labels, int32_t n_genomes, LinkCutoffs q, int64_t &rounds, fa_merge *merges = nullptr,
                            int64_t *n_merges = nullptr) {
  const int64_t n_pairs = front.n_emit; const hipStream_t st = front.st;
  FA_REQUIRE(n_pairs <= (int64_t)(1 << 30), FA_ERR_UNSUPPORTED, "more than 2^30 present pairs");
  StatusBlock<LinkStatus> d_link(st);
  DevBuf<unsigned long long> keys[3];         // the entries to sort, sorted, reduced to distinct keys
  DevBuf<LinkSum> sums[3];
  DevBuf<int32_t> words;                      // seg_start, seg_end, size, parent, best
  DevBuf<unsigned char> temp;
  const size_t n = (size_t)n_genomes;
  words.ensure(n * 5);
  LinkArgs l{};
  l.n_genomes = n_genomes; l.bits = (int32_t)id_bits(n_genomes); l.qm = q.qm; l.qc = q.qc;
  l.seg_start = words.p; l.seg_end = words.p + n; l.size = words.p + 2 * n; l.parent = words.p + 3 * n; l.best = words.p + 4 * n;
  l.labels = labels; l.status = d_link.p;
  const dim3 genome_grid(ceil_div(n_genomes, 256));
  hipLaunchKernelGGL(k_link_init, genome_grid, dim3(256), 0, st, l);
  rounds = 0;
  int64_t n_in = 2 * n_pairs;
  if (n_in) {
    for (int i = 0; i < 3; i++) { keys[i].ensure((size_t)n_in); sums[i].ensure((size_t)n_in); }
    front.emit_link(keys[0].p, sums[0].p);
    l.keys = keys[2].p; l.sums = sums[2].p; l.next_keys = keys[0].p; l.next_sums = sums[0].p;
    // the bits a key can have set: two genome numbers and, above them, the bit of a dropped entry
    const unsigned end_bit = 2u * (unsigned)l.bits + 1u;
    // a round that merges leaves one cluster fewer at least, so at most n_genomes - 1 of them merge
    while (n_in) {
      with_temp(temp, [&](void *t, size_t &bytes) {
        return rocprim::radix_sort_pairs(t, bytes, keys[0].p, keys[1].p, sums[0].p, sums[1].p, (size_t)n_in, 0u, end_bit, st);
      });
      with_temp(temp, [&](void *t, size_t &bytes) {
        return rocprim::reduce_by_key(t, bytes, keys[1].p, sums[1].p, (size_t)n_in, keys[2].p, sums[2].p, &d_link.p->unique, LinkSumPlus(),
                                      rocprim::equal_to<unsigned long long>(), st);
      });
      FA_HIP(hipMemsetAsync(l.seg_start, 0, n * 2 * sizeof(int32_t), st));
      l.bound = n_in; l.round = (unsigned int)rounds + 1u;
      const dim3 entry_grid(ceil_div(n_in, 256));
      hipLaunchKernelGGL(k_link_segments, entry_grid, dim3(256), 0, st, l);
      hipLaunchKernelGGL(k_link_best, genome_grid, dim3(256), 0, st, l);
      if (merges) hipLaunchKernelGGL(k_link_record, genome_grid, dim3(256), 0, st, l, merges, (int64_t)n_genomes - 1);
      hipLaunchKernelGGL(k_link_merge, genome_grid, dim3(256), 0, st, l);
      hipLaunchKernelGGL(k_link_labels, genome_grid, dim3(256), 0, st, l);
      hipLaunchKernelGGL(k_link_relabel, entry_grid, dim3(256), 0, st, l);
      FA_HIP(hipGetLastError());
      const LinkStatus now = d_link.read(st);
      if (now.changed != l.round) break;
      rounds++;
      FA_REQUIRE(rounds < (int64_t)n_genomes, FA_ERR_INTERNAL, "average linkage merged in more rounds than there are genomes");
      n_in = (int64_t)now.live;
    }
  }
  if (merges) {
    const unsigned int recorded = d_link.read(st).merges;
    FA_REQUIRE(!(recorded & LINK_LOST), FA_ERR_INTERNAL, "a merging pair of clusters has no entry in its cluster's run");
    *n_merges = (int64_t)recorded;
  }
  return count_roots(labels, n_genomes, front.d_status.p, st);
}

// whether one label set is valid: every label in [0, n_genomes) and its own label
inline bool label_set_ok(const int32_t *labels, int32_t n_genomes) {
  for (int32_t g = 0; g < n_genomes; g++) {
    const int32_t l = labels[g];
    if (l < 0 || l >= n_genomes || labels[l] != l) return false;
  }
  return true;
}

// The six drivers.  Each reads top to bottom in one order: check_table_args, its own checks, require_device(), the front end
// in its form, its own tail.  A table the front end refuses has therefore touched no output of any of them.
inline void table_pairs(const TableIn &in, fa_pair *pairs, int64_t cap, int64_t *n_pairs, bool pairs_device) {
  check_table_args(in);
  FA_REQUIRE(n_pairs && cap >= 0, FA_ERR_INVALID, "null pair count or negative capacity");
  require_device();
  TableFront front(in, TAB_EMIT_PAIRS);
  *n_pairs = (int64_t)front.status.pairs;                         // (before the capacity check: a caller sizes its buffer by it)
  if (!pairs) return;
  FA_REQUIRE(front.n_emit <= cap, FA_ERR_INVALID, "the pair buffer is smaller than the number of pairs");
  if (!front.n_emit) return;
  Staged<fa_pair> out(pairs, pairs_device, (size_t)front.n_emit);
  front.emit_pairs(out.dev());
  FA_HIP(hipGetLastError());
  out.finish(front.st); FA_HIP(hipStreamSynchronize(front.st));
}

inline void table_clusters(const TableIn &in, int32_t *labels, bool labels_device, int32_t *n_clusters, int64_t *stats) {
  check_table_args(in);
  const int32_t n_genomes = in.n_genomes;
  FA_REQUIRE(n_genomes == 0 || labels, FA_ERR_INVALID, "null labels");
  require_device();
  TableFront front(in, TAB_EMIT_EDGES);
  int64_t rounds = 0; unsigned int roots = 0;
  if (n_genomes) {
    DevBuf<int2> d_edges;
    Staged<int32_t> out(labels, labels_device, (size_t)n_genomes);
    d_edges.ensure((size_t)front.n_emit);
    front.emit_edges(d_edges.p);
    roots = components(d_edges.p, front.n_emit, out.dev(), n_genomes, front.d_status.p, front.st, rounds);
    out.finish(front.st); FA_HIP(hipStreamSynchronize(front.st));
  }
  if (n_clusters) *n_clusters = (int32_t)roots;
  front.write_stats(stats, rounds);
}

inline void table_representatives(const TableIn &in, const int32_t *order, int32_t *labels, double *identity, bool out_device,
                                  int32_t *n_representatives, int64_t *stats) {
  check_table_args(in);
  const int32_t n_genomes = in.n_genomes;
  FA_REQUIRE(n_genomes == 0 || labels, FA_ERR_INVALID, "null labels");
  FA_REQUIRE(in.p->min_identity >= 0.0f, FA_ERR_INVALID, "min_identity must be a number that is not negative");          // (false for NaN)
  std::vector<int32_t> both;                  // pos, then order
  FA_REQUIRE(order_positions(order, n_genomes, both), FA_ERR_INVALID, "order is not a permutation of the genome numbers");
  require_device();
  TableFront front(in, TAB_EMIT_WEIGHTED);
  int64_t rounds = 0; unsigned int roots = 0;
  if (n_genomes) {
    DevBuf<TableEdge> d_edges; DevBuf<int32_t> d_order;
    both.resize((size_t)n_genomes * 2);
    for (int32_t g = 0; g < n_genomes; g++) both[(size_t)n_genomes + (size_t)both[(size_t)g]] = g;
    d_order.upload(both, front.st);
    Staged<int32_t> out(labels, out_device, (size_t)n_genomes);
    Staged<double> out_identity(identity, out_device, (size_t)n_genomes);
    d_edges.ensure((size_t)front.n_emit);
    front.emit_weighted(d_edges.p);
    roots = representatives(d_edges.p, front.n_emit, d_order.p, d_order.p + n_genomes, out.dev(), out_identity.dev(), n_genomes,
                            front.d_status.p, front.st, rounds);
    out.finish(front.st); out_identity.finish(front.st);
    FA_HIP(hipStreamSynchronize(front.st));
  }
  if (n_representatives) *n_representatives = (int32_t)roots;
  front.write_stats(stats, rounds);
}

inline void table_linkage(const TableIn &in, float missing, int32_t *labels, bool labels_device, int32_t *n_clusters, int64_t *stats) {
  check_table_args(in);
  const int32_t n_genomes = in.n_genomes;
  FA_REQUIRE(n_genomes == 0 || labels, FA_ERR_INVALID, "null labels");
  const LinkCutoffs q = check_linkage_args(in.p, missing, n_genomes);
  require_device();
  TableFront front(in, TAB_EMIT_LINK);
  int64_t rounds = 0; unsigned int roots = 0;
  if (n_genomes) {
    Staged<int32_t> out(labels, labels_device, (size_t)n_genomes);
    roots = linkage(front, out.dev(), n_genomes, q, rounds);
    out.finish(front.st); FA_HIP(hipStreamSynchronize(front.st));
  }
  if (n_clusters) *n_clusters = (int32_t)roots;
  front.write_stats(stats, rounds);
  if (stats) stats[4] = (int64_t)n_genomes - (int64_t)roots;
}

// fa_table_dendrogram: `labels` may be null, and out_device holds for merges and labels
inline void table_dendrogram(const TableIn &in, float missing, fa_merge *merges, int64_t cap, int64_t *n_merges, int32_t *labels, bool out_device,
                             int32_t *n_clusters, int64_t *stats) {
  check_table_args(in);
  const int32_t n_genomes = in.n_genomes;
  FA_REQUIRE(n_merges && (!merges || cap >= 0), FA_ERR_INVALID, "null merge count or negative capacity");
  const LinkCutoffs q = check_linkage_args(in.p, missing, n_genomes);
  require_device();
  TableFront front(in, TAB_EMIT_LINK);
  const hipStream_t st = front.st;
  // everything lands in buffers of the call's own first: a short `cap` leaves the caller's memory as it was
  int64_t rounds = 0, n_found = 0; unsigned int roots = 0;
  DevBuf<int32_t> d_labels, order;             // order: the records' numbers in the order of the walk
  DevBuf<fa_merge> found, sorted;
  if (n_genomes) {
    d_labels.ensure((size_t)n_genomes);
    found.ensure((size_t)std::max(n_genomes - 1, 1));
    roots = linkage(front, d_labels.p, n_genomes, q, rounds, found.p, &n_found);
    FA_REQUIRE(n_found == (int64_t)n_genomes - (int64_t)roots, FA_ERR_INTERNAL, "the merge list and the labels disagree on the number of merges");
  }
  *n_merges = n_found;                                            // (before the capacity check, as fa_table_pairs)
  FA_REQUIRE(!merges || n_found <= cap, FA_ERR_INVALID, "the merge buffer is smaller than the number of merges");
  const hipMemcpyKind kind = out_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (merges && n_found) {
    // the order of the walk (fa_linkage.hip.h): total on the records, so the bytes do not depend on the slots they were taken in
    sorted.ensure((size_t)n_found); order.ensure((size_t)n_found);
    with_temp(front.temp, [&](void *t, size_t &bytes) {
      return rocprim::merge_sort(t, bytes, rocprim::counting_iterator<int32_t>(0), order.p, (size_t)n_found, MergeIndexBefore{found.p}, st);
    });
    hipLaunchKernelGGL(k_link_gather, dim3(ceil_div(n_found, 256)), dim3(256), 0, st, (const fa_merge *)found.p, (const int32_t *)order.p, n_found,
                       sorted.p);
    FA_HIP(hipGetLastError());
    FA_HIP(hipMemcpyAsync(merges, sorted.p, (size_t)n_found * sizeof(fa_merge), kind, st));
  }
  if (labels && n_genomes) FA_HIP(hipMemcpyAsync(labels, d_labels.p, (size_t)n_genomes * sizeof(int32_t), kind, st));
  FA_HIP(hipStreamSynchronize(st));
  if (n_clusters) *n_clusters = (int32_t)roots;
  front.write_stats(stats, rounds);
  if (stats) stats[4] = (int64_t)n_genomes - (int64_t)roots;
}

// fa_table_medoids (fa_medoid.hip.h): labels and the four outputs, each [n_sets][n_genomes], are the caller's device pointers
// with io_device; n_clusters [n_sets] is host memory
inline void table_medoids(const TableIn &in, float missing, const int32_t *labels, int32_t n_sets, const double *bonus, int32_t *medoids,
                          double *identity, int64_t *sums, int32_t *sizes, bool io_device, int32_t *n_clusters, int64_t *stats) {
  check_table_args(in);
  const int32_t n_genomes = in.n_genomes;
  FA_REQUIRE(missing >= 0.0f && missing <= (float)LINK_MAX_IDENTITY, FA_ERR_INVALID, "missing must be a number in [0, 128]");   // (false for NaN)
  FA_REQUIRE(n_sets >= 1, FA_ERR_INVALID, "medoids need at least one label set");
  FA_REQUIRE(n_genomes == 0 || labels, FA_ERR_INVALID, "null labels");
  FA_REQUIRE(n_genomes <= LINK_MAX_GENOMES, FA_ERR_UNSUPPORTED, "medoids over more than 2^18 genomes");
  FA_REQUIRE((int64_t)n_sets * (int64_t)n_genomes <= (int64_t)INT32_MAX, FA_ERR_UNSUPPORTED, "more than 2^31 - 1 labels");
  std::vector<long long> qb;                   // empty for no bonus
  if (bonus) {
    qb.resize((size_t)n_genomes);
    for (int32_t g = 0; g < n_genomes; g++) {
      FA_REQUIRE(medoid_bonus_ok(bonus[g]), FA_ERR_INVALID, "a bonus must be a number in [-32768, 32768]");
      qb[(size_t)g] = medoid_qb(bonus[g]);
    }
  }
  // (labels on the host are checked here, those in HBM by k_medoid_check -- which sees the host's again)
  if (!io_device)
    for (int32_t t = 0; t < n_sets; t++)
      FA_REQUIRE(label_set_ok(labels + (size_t)t * (size_t)n_genomes, n_genomes), FA_ERR_INVALID,
                 "a label lies outside [0, n_genomes) or is not its own label");
  require_device();
  TableFront front(in, TAB_EMIT_LINK);
  const hipStream_t st = front.st;
  if (!n_genomes) {
    if (n_clusters) std::fill(n_clusters, n_clusters + n_sets, 0);
    front.write_stats(stats, 0);
    return;
  }
  FA_REQUIRE(front.n_emit <= (int64_t)(1 << 30), FA_ERR_UNSUPPORTED, "more than 2^30 present pairs");
  StatusBlock<MedoidStatus> d_status(st);
  DevBuf<int32_t> d_labels, words;            // words: seg_start, seg_end, then size and who of every (set, genome)
  DevBuf<unsigned long long> keys[2], best;
  DevBuf<LinkSum> entry_sums[2];
  DevBuf<long long> s, d_qb;
  DevBuf<unsigned int> d_roots;
  DevBuf<unsigned char> temp;
  const size_t n = (size_t)n_genomes, total = n * (size_t)n_sets;
  const int64_t n_in = 2 * front.n_emit;

  MedoidArgs a{};
  a.n_entries = n_in; a.n_genomes = n_genomes; a.n_sets = n_sets; a.bits = (int32_t)id_bits(n_genomes); a.qm = link_fixed((double)missing);
  a.status = d_status.p;
  a.labels = on_device(labels, io_device, total, d_labels, st);
  words.ensure(2 * n + 2 * total);
  a.seg_start = words.p; a.seg_end = words.p + n; a.size = words.p + 2 * n; a.who = words.p + 2 * n + total;
  FA_HIP(hipMemsetAsync(words.p, 0, (2 * n + total) * sizeof(int32_t), st));
  FA_HIP(hipMemsetAsync(a.who, 0x7F, total * sizeof(int32_t), st));            // 0x7F7F7F7F: above every genome number
  const dim3 grid((unsigned)ceil_div(n_genomes, 256), (unsigned)std::min(n_sets, 65535));
  // the verdict on the labels is read before they index anything and before an output is touched
  hipLaunchKernelGGL(k_medoid_check, grid, dim3(256), 0, st, a);
  FA_HIP(hipGetLastError());
  FA_REQUIRE(!(d_status.read(st).flags & MED_BAD_LABEL), FA_ERR_INVALID,
             "a label lies outside [0, n_genomes) or is not its own label");
  if (n_in) {
    for (int i = 0; i < 2; i++) { keys[i].ensure((size_t)n_in); entry_sums[i].ensure((size_t)n_in); }
    front.emit_link(keys[0].p, entry_sums[0].p);
    // one sort for all the sets; the bits a key can have set: two genome numbers
    const unsigned end_bit = 2u * (unsigned)a.bits;
    with_temp(temp, [&](void *t, size_t &bytes) {
      return rocprim::radix_sort_pairs(t, bytes, keys[0].p, keys[1].p, entry_sums[0].p, entry_sums[1].p, (size_t)n_in, 0u, end_bit, st);
    });
    a.keys = keys[1].p; a.sums = entry_sums[1].p;
    hipLaunchKernelGGL(k_medoid_segments, dim3(ceil_div(n_in, 256)), dim3(256), 0, st, a);
  }
  s.ensure(total);
  a.s = s.p;
  const dim3 sums_grid(grid.x, (unsigned)std::min(ceil_div(n_sets, MED_SETS), 65535));
  hipLaunchKernelGGL(k_medoid_sums, sums_grid, dim3(256), 0, st, a);
  if (!qb.empty()) { d_qb.upload(qb, st); a.qb = d_qb.p; }
  best.ensure(total);
  FA_HIP(hipMemsetAsync(best.p, 0, total * sizeof(unsigned long long), st));
  a.best = best.p;
  hipLaunchKernelGGL(k_medoid_best, grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_medoid_pick, grid, dim3(256), 0, st, a);
  d_roots.ensure((size_t)n_sets);
  FA_HIP(hipMemsetAsync(d_roots.p, 0, (size_t)n_sets * sizeof(unsigned int), st));
  a.roots = d_roots.p;
  Staged<int32_t> out_medoids(medoids, io_device, total), out_sizes(sizes, io_device, total);
  Staged<double> out_identity(identity, io_device, total);
  Staged<int64_t> out_sums(sums, io_device, total);
  a.medoids = out_medoids.dev(); a.identity = out_identity.dev(); a.sums_out = out_sums.dev(); a.sizes_out = out_sizes.dev();
  hipLaunchKernelGGL(k_medoid_write, grid, dim3(256), 0, st, a);
  FA_HIP(hipGetLastError());
  out_medoids.finish(st); out_identity.finish(st); out_sums.finish(st); out_sizes.finish(st);
  std::vector<unsigned int> roots((size_t)n_sets, 0u);
  d_roots.download(roots.data(), roots.size(), st);
  const int64_t inside = (int64_t)(d_status.read(st).inside / 2ULL);            // (two directed entries a pair; read() synchronises)
  if (n_clusters) for (int32_t t = 0; t < n_sets; t++) n_clusters[t] = (int32_t)roots[(size_t)t];
  front.write_stats(stats, inside);
}

// The partitions of a merge list at n_cuts cut-offs (fa_dendrogram_cut; fa_linkage.hip.h has the road)
inline void dendrogram_cut(const fa_merge *merges, int64_t n_merges, bool merges_device, int32_t n_genomes, const float *min_identity,
                           int32_t n_cuts, int32_t *labels, bool labels_device, int32_t *n_clusters) {
  FA_REQUIRE(n_cuts >= 1 && min_identity, FA_ERR_INVALID, "a cut needs at least one cut-off");
  FA_REQUIRE(n_genomes >= 0, FA_ERR_INVALID, "negative number of genomes");
  FA_REQUIRE(n_merges >= 0 && n_merges <= (int64_t)std::max(n_genomes - 1, 0), FA_ERR_INVALID, "the number of merges lies outside [0, n_genomes - 1]");
  FA_REQUIRE(n_merges == 0 || merges, FA_ERR_INVALID, "null merges");
  FA_REQUIRE(n_genomes == 0 || labels, FA_ERR_INVALID, "null labels");
  std::vector<long long> qc((size_t)n_cuts);
  for (int32_t t = 0; t < n_cuts; t++) {
    FA_REQUIRE(min_identity[t] >= 0.0f, FA_ERR_INVALID, "min_identity must be a number that is not negative");          // (false for NaN)
    qc[(size_t)t] = link_cutoff(min_identity[t]);
  }
  FA_REQUIRE(n_genomes <= LINK_MAX_GENOMES, FA_ERR_UNSUPPORTED, "average linkage over more than 2^18 genomes");
  FA_REQUIRE((int64_t)n_cuts * (int64_t)n_genomes <= (int64_t)INT32_MAX, FA_ERR_UNSUPPORTED, "more than 2^31 - 1 labels");
  require_device();
  if (!n_genomes) {
    if (n_clusters) std::fill(n_clusters, n_clusters + n_cuts, 0);
    return;
  }
  CallStream stream;
  hipStream_t st = stream.s;
  StatusBlock<CutStatus> d_status(st);
  DevBuf<fa_merge> d_merges;
  DevBuf<long long> d_qc;
  DevBuf<int32_t> slot, other;
  DevBuf<unsigned int> d_roots;
  const size_t n = (size_t)n_genomes, total = n * (size_t)n_cuts;

  CutArgs a{};
  a.n_merges = n_merges; a.n_genomes = n_genomes; a.n_cuts = n_cuts; a.status = d_status.p;
  slot.ensure(n);
  FA_HIP(hipMemsetAsync(slot.p, 0xFF, n * sizeof(int32_t), st));
  a.slot = slot.p;
  if (n_merges) {
    // the verdict on the list is read before an output is touched
    a.merges = on_device(merges, merges_device, (size_t)n_merges, d_merges, st);
    const dim3 merge_grid(ceil_div(n_merges, 256));
    hipLaunchKernelGGL(k_cut_check, merge_grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_cut_twice, merge_grid, dim3(256), 0, st, a);
    FA_HIP(hipGetLastError());
    const CutStatus status = d_status.read(st);
    FA_REQUIRE(!(status.flags & CUT_BAD_MERGE), FA_ERR_INVALID,
               "a merge is not 0 <= lo < hi < n_genomes with sizes >= 1 that add up to n_genomes at most, s >= 0 and present >= 1");
    FA_REQUIRE(!(status.flags & CUT_TWICE), FA_ERR_INVALID, "a label is merged away twice: the same hi in two merges");
  }
  d_qc.upload(qc, st);
  a.qc = d_qc.p;
  // round r reads buffer (r - 1) % 2 and writes buffer r % 2 (k_cut_parent writes buffer 0): the last one is the output
  const int rounds = (int)bit_width_u64((unsigned long long)(n_genomes - 1));
  Staged<int32_t> out(labels, labels_device, total);
  other.ensure(total);
  int32_t *buffer[2];
  buffer[rounds % 2] = out.dev();
  buffer[1 - rounds % 2] = other.p;
  const dim3 grid((unsigned)ceil_div(n_genomes, 256), (unsigned)std::min(n_cuts, 65535));
  hipLaunchKernelGGL(k_cut_parent, grid, dim3(256), 0, st, a, buffer[0]);
  for (int r = 1; r <= rounds; r++)
    hipLaunchKernelGGL(k_cut_jump, grid, dim3(256), 0, st, (const int32_t *)buffer[(r - 1) % 2], buffer[r % 2], n_genomes, n_cuts);
  std::vector<unsigned int> roots;
  if (n_clusters) {
    d_roots.ensure((size_t)n_cuts);
    FA_HIP(hipMemsetAsync(d_roots.p, 0, (size_t)n_cuts * sizeof(unsigned int), st));
    a.roots = d_roots.p;
    hipLaunchKernelGGL(k_cut_roots, grid, dim3(256), 0, st, a, (const int32_t *)out.dev());
    roots.resize((size_t)n_cuts);
    d_roots.download(roots.data(), roots.size(), st);
  }
  FA_HIP(hipGetLastError());
  out.finish(st);
  FA_HIP(hipStreamSynchronize(st));
  for (size_t t = 0; t < roots.size(); t++) n_clusters[t] = (int32_t)roots[t];
}

// ------------------------------------------------------------------------------------------------------------
// The fragment mappings behind a hit table reduced to a per-fragment profile (fa_profile.hip.h has the semantics and the road)
// ------------------------------------------------------------------------------------------------------------
// the road of k_profile_add: 0 the policy, 1 global atomics only, 2 on chip wherever it fits (fa_debug_profile_road)
inline std::atomic<int> g_profile_road{0};

// fragment_offsets as both calls take it: [n_queries + 1], from 0, never decreasing
inline void check_fragment_offsets(int32_t n_queries, const int64_t *fragment_offsets) {
  FA_REQUIRE(n_queries >= 0, FA_ERR_INVALID, "negative number of queries");
  FA_REQUIRE(fragment_offsets, FA_ERR_INVALID, "null fragment offsets");
  FA_REQUIRE(fragment_offsets[0] == 0, FA_ERR_INVALID, "fragment_offsets must start at 0");
  for (int32_t q = 0; q < n_queries; q++)
    FA_REQUIRE(fragment_offsets[q + 1] >= fragment_offsets[q], FA_ERR_INVALID, "fragment_offsets must not decrease");
}

// fa_mappings_profile: the three accumulators are the caller's device arrays; offsets, labels and self_reference host arrays
inline void mappings_profile(const fa_hit_mapping *maps, int64_t n_maps, bool maps_device, int32_t n_queries, const int64_t *fragment_offsets,
                             int32_t n_references, const int32_t *query_labels, const int32_t *reference_labels, const int32_t *self_reference,
                             float min_identity, int32_t *d_count, int64_t *d_sum, float *d_lowest, int64_t *stats) {
  FA_REQUIRE(n_maps >= 0 && n_references >= 0, FA_ERR_INVALID, "negative number of records or references");
  check_fragment_offsets(n_queries, fragment_offsets);
  FA_REQUIRE(n_maps == 0 || maps, FA_ERR_INVALID, "null records");
  FA_REQUIRE((query_labels != nullptr) == (reference_labels != nullptr), FA_ERR_INVALID, "query_labels and reference_labels go together");
  FA_REQUIRE(min_identity == min_identity, FA_ERR_INVALID, "min_identity must be a number");
  const int64_t total = fragment_offsets[n_queries];
  FA_REQUIRE(total == 0 || (d_count && d_sum && d_lowest), FA_ERR_INVALID, "null accumulators");
  const int64_t n_chunks = (n_maps + PROF_CHUNK - 1) / PROF_CHUNK;
  FA_REQUIRE(n_chunks <= (int64_t)INT32_MAX, FA_ERR_UNSUPPORTED, "more than 2^31 - 1 chunks of records");
  require_device();
  if (!n_maps) {
    if (stats) std::fill(stats, stats + 4, (int64_t)0);
    return;
  }
  CallStream stream;
  hipStream_t st = stream.s;
  StatusBlock<ProfileStatus> d_status(st);
  DevBuf<fa_hit_mapping> d_maps;
  DevBuf<int64_t> d_offsets;
  DevBuf<int32_t> words, chunk_query;          // words: query_labels, reference_labels, self_reference

  ProfileArgs a{};
  a.maps = reinterpret_cast<const int4 *>(on_device(maps, maps_device, (size_t)n_maps, d_maps, st));
  a.n_maps = n_maps; a.n_queries = n_queries; a.n_references = n_references; a.min_identity = min_identity;
  d_offsets.upload(fragment_offsets, (size_t)n_queries + 1, st);
  a.offsets = d_offsets.p;
  const size_t nq = (size_t)n_queries, nr = (size_t)n_references;
  words.ensure(2 * nq + nr);
  if (query_labels) {
    if (nq) FA_HIP(hipMemcpyAsync(words.p, query_labels, nq * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (nr) FA_HIP(hipMemcpyAsync(words.p + nq, reference_labels, nr * sizeof(int32_t), hipMemcpyHostToDevice, st));
    a.query_labels = words.p; a.reference_labels = words.p + nq;
  }
  if (self_reference) {
    if (nq) FA_HIP(hipMemcpyAsync(words.p + nq + nr, self_reference, nq * sizeof(int32_t), hipMemcpyHostToDevice, st));
    a.self_reference = words.p + nq + nr;
  }
  chunk_query.ensure((size_t)n_chunks);
  a.chunk_query = chunk_query.p;
  a.count = d_count; a.sum = reinterpret_cast<unsigned long long *>(d_sum); a.lowest = reinterpret_cast<unsigned int *>(d_lowest);
  a.status = d_status.p;
  const int road = g_profile_road.load();
  a.road = road ? road : (PROF_POLICY_ON_CHIP ? 2 : 1);
  // the verdict on the records is read before an accumulator is touched
  hipLaunchKernelGGL(k_profile_check, dim3((unsigned)n_chunks), dim3(PROF_THREADS), 0, st, a);
  FA_HIP(hipGetLastError());
  const ProfileStatus checked = d_status.read(st);
  FA_REQUIRE(!(checked.flags & PROF_BAD_QUERY), FA_ERR_INVALID, "a record names a query outside [0, n_queries)");
  FA_REQUIRE(!(checked.flags & PROF_BAD_FRAGMENT), FA_ERR_INVALID, "a record names a fragment outside its query's fragments");
  FA_REQUIRE(!(checked.flags & PROF_BAD_REFERENCE), FA_ERR_INVALID, "a record names a reference outside [0, n_references)");
  FA_REQUIRE(!(checked.flags & PROF_BAD_IDENTITY), FA_ERR_INVALID, "a record's identity is NaN, negative (-0.0 included) or above 128");
  hipLaunchKernelGGL(k_profile_add, dim3((unsigned)n_chunks), dim3(PROF_THREADS), 0, st, a);
  FA_HIP(hipGetLastError());
  const ProfileStatus end = d_status.read(st);
  if (stats) { stats[0] = (int64_t)end.counted; stats[1] = (int64_t)end.skipped; stats[2] = (int64_t)end.below; stats[3] = (int64_t)end.on_chip; }
}

// fa_profile_summary: d_count and d_sum are device arrays; min_count [n_sets][n_queries] is host memory; the three outputs,
// each [n_sets][n_queries] or null, are device pointers with out_device
inline void profile_summary(const int32_t *d_count, const int64_t *d_sum, int32_t n_queries, const int64_t *fragment_offsets,
                            const int32_t *min_count, int32_t n_sets, int64_t *fragments, int64_t *hits, int64_t *sum, bool out_device) {
  check_fragment_offsets(n_queries, fragment_offsets);
  FA_REQUIRE(n_sets >= 1, FA_ERR_INVALID, "a summary needs at least one threshold set");
  FA_REQUIRE(n_queries == 0 || min_count, FA_ERR_INVALID, "null min_count");
  FA_REQUIRE(fragment_offsets[n_queries] == 0 || (d_count && d_sum), FA_ERR_INVALID, "null accumulators");
  FA_REQUIRE((int64_t)n_sets * (int64_t)n_queries <= (int64_t)INT32_MAX, FA_ERR_UNSUPPORTED, "more than 2^31 - 1 thresholds");
  const size_t total = (size_t)n_sets * (size_t)n_queries;
  for (size_t i = 0; i < total; i++) FA_REQUIRE(min_count[i] >= 0, FA_ERR_INVALID, "min_count must not be negative");
  require_device();
  if (!n_queries) return;
  CallStream stream;
  hipStream_t st = stream.s;
  DevBuf<int64_t> d_offsets;
  DevBuf<int32_t> d_min;
  d_offsets.upload(fragment_offsets, (size_t)n_queries + 1, st);
  d_min.upload(min_count, total, st);
  Staged<int64_t> out_fragments(fragments, out_device, total), out_hits(hits, out_device, total), out_sum(sum, out_device, total);
  SummaryArgs a{};
  a.count = d_count; a.sum = reinterpret_cast<const long long *>(d_sum); a.offsets = d_offsets.p; a.min_count = d_min.p;
  a.n_queries = n_queries; a.n_sets = n_sets;
  a.fragments = out_fragments.dev(); a.hits = out_hits.dev(); a.sums = out_sum.dev();
  const dim3 grid((unsigned)n_queries, (unsigned)std::min(ceil_div(n_sets, PROF_SETS), 65535));
  hipLaunchKernelGGL(k_profile_summary, grid, dim3(PROF_THREADS), 0, st, a);
  FA_HIP(hipGetLastError());
  out_fragments.finish(st); out_hits.finish(st); out_sum.finish(st);
  FA_HIP(hipStreamSynchronize(st));
}

// fa_mappings_reference_profile: the three accumulators are the caller's device arrays; contig_bin, contig_genome, labels and
// self_reference host arrays (fa_refprofile.hip.h has the semantics and the road)
inline void mappings_reference_profile(const fa_hit_mapping *maps, int64_t n_maps, bool maps_device, int32_t n_queries, int32_t n_references,
                                       int32_t n_contigs, const int32_t *contig_bin, const int32_t *contig_genome, int32_t bin_length,
                                       const int32_t *query_labels, const int32_t *reference_labels, const int32_t *self_reference,
                                       float min_identity, int32_t *d_count, int64_t *d_sum, float *d_lowest, int64_t *stats) {
  FA_REQUIRE(n_maps >= 0 && n_references >= 0 && n_queries >= 0 && n_contigs >= 0, FA_ERR_INVALID,
             "negative number of records, queries, references or contigs");
  FA_REQUIRE(bin_length >= 1, FA_ERR_INVALID, "bin_length must be at least 1");
  FA_REQUIRE(contig_bin && (n_contigs == 0 || contig_genome), FA_ERR_INVALID, "null contig_bin or contig_genome");
  FA_REQUIRE(contig_bin[0] == 0, FA_ERR_INVALID, "contig_bin must start at 0");
  for (int32_t c = 0; c < n_contigs; c++) {
    FA_REQUIRE(contig_bin[c + 1] >= contig_bin[c], FA_ERR_INVALID, "contig_bin must not decrease");
    FA_REQUIRE(contig_genome[c] >= (c ? contig_genome[c - 1] : 0) && contig_genome[c] < n_references, FA_ERR_INVALID,
               "contig_genome must not decrease and must stay inside [0, n_references)");
  }
  FA_REQUIRE(n_maps == 0 || maps, FA_ERR_INVALID, "null records");
  FA_REQUIRE((query_labels != nullptr) == (reference_labels != nullptr), FA_ERR_INVALID, "query_labels and reference_labels go together");
  FA_REQUIRE(min_identity == min_identity, FA_ERR_INVALID, "min_identity must be a number");
  FA_REQUIRE(contig_bin[n_contigs] == 0 || (d_count && d_sum && d_lowest), FA_ERR_INVALID, "null accumulators");
  const int64_t n_chunks = (n_maps + REFPROF_CHUNK - 1) / REFPROF_CHUNK;
  FA_REQUIRE(n_chunks <= (int64_t)INT32_MAX, FA_ERR_UNSUPPORTED, "more than 2^31 - 1 chunks of records");
  require_device();
  if (!n_maps) {
    if (stats) std::fill(stats, stats + 3, (int64_t)0);
    return;
  }
  CallStream stream;
  hipStream_t st = stream.s;
  StatusBlock<ProfileStatus> d_status(st);
  DevBuf<fa_hit_mapping> d_maps;
  DevBuf<int32_t> words;          // contig_bin, contig_genome, query_labels, reference_labels, self_reference

  RefProfileArgs a{};
  a.maps = reinterpret_cast<const int4 *>(on_device(maps, maps_device, (size_t)n_maps, d_maps, st));
  a.n_maps = n_maps; a.n_queries = n_queries; a.n_references = n_references; a.n_contigs = n_contigs;
  a.bin_length = bin_length; a.min_identity = min_identity;
  const size_t nq = (size_t)n_queries, nr = (size_t)n_references, nc = (size_t)n_contigs;
  words.ensure(2 * nc + 1 + 2 * nq + nr);
  int32_t *at = words.p;
  const auto put = [&](const int32_t *host, size_t n) {
    int32_t *where = at;
    if (n) FA_HIP(hipMemcpyAsync(where, host, n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    at += n;
    return where;
  };
  a.contig_bin = put(contig_bin, nc + 1);
  a.contig_genome = put(contig_genome, nc);
  if (query_labels) { a.query_labels = put(query_labels, nq); a.reference_labels = put(reference_labels, nr); }
  if (self_reference) a.self_reference = put(self_reference, nq);
  a.count = d_count; a.sum = reinterpret_cast<unsigned long long *>(d_sum); a.lowest = reinterpret_cast<unsigned int *>(d_lowest);
  a.status = d_status.p;
  // the verdict on the records is read before an accumulator is touched
  hipLaunchKernelGGL(k_refprofile_check, dim3((unsigned)n_chunks), dim3(REFPROF_THREADS), 0, st, a);
  FA_HIP(hipGetLastError());
  const ProfileStatus checked = d_status.read(st);
  FA_REQUIRE(!(checked.flags & PROF_BAD_QUERY), FA_ERR_INVALID, "a record names a query outside [0, n_queries)");
  FA_REQUIRE(!(checked.flags & PROF_BAD_REFERENCE), FA_ERR_INVALID, "a record names a reference outside [0, n_references)");
  FA_REQUIRE(!(checked.flags & PROF_BAD_CONTIG), FA_ERR_INVALID, "a record names a contig outside [0, n_contigs)");
  FA_REQUIRE(!(checked.flags & PROF_BAD_CONTIG_GENOME), FA_ERR_INVALID, "a record's contig belongs to another reference genome");
  FA_REQUIRE(!(checked.flags & PROF_BAD_POSITION), FA_ERR_INVALID, "a record's position is negative or outside the bins of its contig");
  FA_REQUIRE(!(checked.flags & PROF_BAD_IDENTITY), FA_ERR_INVALID, "a record's identity is NaN, negative (-0.0 included) or above 128");
  hipLaunchKernelGGL(k_refprofile_add, dim3((unsigned)n_chunks), dim3(REFPROF_THREADS), 0, st, a);
  FA_HIP(hipGetLastError());
  FA_HIP(hipStreamSynchronize(st));
  if (stats) { stats[0] = (int64_t)checked.counted; stats[1] = (int64_t)checked.skipped; stats[2] = (int64_t)checked.below; }
}

// fa_profile_regions: d_count and d_sum are device arrays; segment_offsets and need host arrays; `regions` is a device pointer
// with out_device
inline void profile_regions(const int32_t *d_count, const int64_t *d_sum, int32_t n_segments, const int64_t *segment_offsets,
                            const int32_t *need, bool below, int32_t min_length, fa_profile_region *regions, int64_t cap,
                            int64_t *n_regions, bool out_device) {
  check_fragment_offsets(n_segments, segment_offsets);
  FA_REQUIRE(min_length >= 1, FA_ERR_INVALID, "min_length must be at least 1");
  FA_REQUIRE(n_segments == 0 || need, FA_ERR_INVALID, "null need");
  for (int32_t s = 0; s < n_segments; s++) FA_REQUIRE(need[s] >= 0, FA_ERR_INVALID, "need must not be negative");
  const int64_t total = segment_offsets[n_segments];
  FA_REQUIRE(total == 0 || d_count, FA_ERR_INVALID, "null count");
  FA_REQUIRE(!regions || cap >= 0, FA_ERR_INVALID, "negative capacity");
  FA_REQUIRE(total <= (int64_t)INT32_MAX, FA_ERR_UNSUPPORTED, "a profile of more than 2^31 - 1 entries");
  require_device();
  if (!total) {
    if (n_regions) *n_regions = 0;
    return;
  }
  CallStream stream;
  hipStream_t st = stream.s;
  StatusBlock<RegionStatus> d_status(st);
  DevBuf<int64_t> d_offsets, offs;
  DevBuf<int32_t> d_need, counts, runs;
  DevBuf<unsigned long long> before;
  DevBuf<unsigned char> temp;

  RegionArgs a{};
  a.count = d_count; a.sum = reinterpret_cast<const unsigned long long *>(d_sum);
  d_offsets.upload(segment_offsets, (size_t)n_segments + 1, st);
  d_need.upload(need, (size_t)n_segments, st);
  a.offsets = d_offsets.p; a.need = d_need.p;
  a.n_segments = n_segments; a.total = (int32_t)total; a.below = below ? 1 : 0; a.min_length = min_length;
  const int32_t n_chunks = (int32_t)ceil_div(total, (int64_t)REG_CHUNK);
  counts.ensure(2 * (size_t)n_chunks); offs.ensure(2 * (size_t)n_chunks);
  a.chunk_starts = counts.p; a.chunk_ends = counts.p + n_chunks;
  a.start_off = offs.p; a.end_off = offs.p + n_chunks;
  hipLaunchKernelGGL(k_region_runs<false>, dim3((unsigned)n_chunks), dim3(REG_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_chunk_scan, dim3(1), dim3(1024), 0, st, a.chunk_starts, a.start_off, n_chunks, &d_status.p->starts);
  hipLaunchKernelGGL(k_chunk_scan, dim3(1), dim3(1024), 0, st, a.chunk_ends, a.end_off, n_chunks, &d_status.p->ends);
  FA_HIP(hipGetLastError());
  const RegionStatus found = d_status.read(st);
  FA_REQUIRE(found.starts == found.ends, FA_ERR_INTERNAL, "the starts and the ends of the runs do not pair up");
  a.n_runs = found.starts;
  int64_t n_records = 0;
  DevBuf<int32_t> kept;
  DevBuf<int64_t> kept_off;
  const int32_t n_run_chunks = (int32_t)ceil_div(a.n_runs, (int64_t)REG_CHUNK);
  if (a.n_runs) {
    runs.ensure(3 * (size_t)a.n_runs);
    a.run_segment = runs.p; a.run_first = runs.p + a.n_runs; a.run_last = runs.p + 2 * a.n_runs;
    hipLaunchKernelGGL(k_region_runs<true>, dim3((unsigned)n_chunks), dim3(REG_THREADS), 0, st, a);
    kept.ensure((size_t)n_run_chunks); kept_off.ensure((size_t)n_run_chunks);
    a.chunk_kept = kept.p; a.kept_off = kept_off.p;
    hipLaunchKernelGGL(k_region_emit<false>, dim3((unsigned)n_run_chunks), dim3(REG_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_chunk_scan, dim3(1), dim3(1024), 0, st, a.chunk_kept, a.kept_off, n_run_chunks, &d_status.p->regions);
    FA_HIP(hipGetLastError());
    n_records = d_status.read(st).regions;
  }
  if (n_regions) *n_regions = n_records;
  FA_REQUIRE(!regions || n_records <= cap, FA_ERR_INVALID, "the region buffer is smaller than the number of regions");
  if (!regions || !n_records) return;
  // hits and sum of a run: differences of the exclusive sums of count and of sum over the whole profile
  before.ensure(2 * (size_t)total);
  unsigned long long *count_before = before.p, *sum_before = before.p + total;
  with_temp(temp, [&](void *t, size_t &bytes) {
    return rocprim::exclusive_scan(t, bytes, rocprim::make_transform_iterator(d_count, CountAsU64()), count_before, 0ULL, (size_t)total,
                                   rocprim::plus<unsigned long long>(), st);
  });
  if (a.sum)
    with_temp(temp, [&](void *t, size_t &bytes) {
      return rocprim::exclusive_scan(t, bytes, a.sum, sum_before, 0ULL, (size_t)total, rocprim::plus<unsigned long long>(), st);
    });
  a.count_before = count_before; a.sum_before = sum_before;
  Staged<fa_profile_region> out(regions, out_device, (size_t)n_records);
  a.regions = reinterpret_cast<RegionRecord *>(out.dev());
  hipLaunchKernelGGL(k_region_emit<true>, dim3((unsigned)n_run_chunks), dim3(REG_THREADS), 0, st, a);
  FA_HIP(hipGetLastError());
  out.finish(st);
  FA_HIP(hipStreamSynchronize(st));
}

// ------------------------------------------------------------------------------------------------------------
// A query x reference hit table reduced to every query's k best hits (fa_best.hip.h has the semantics and the road)
// ------------------------------------------------------------------------------------------------------------
inline void table_best(const fa_cgi_row *rows, int64_t n_rows, bool rows_device, int32_t n_queries, int32_t n_references,
                       const uint64_t *query_lengths, const uint64_t *reference_lengths, const fa_best_params *p, fa_cgi_row *best,
                       int64_t *offsets, int64_t cap, int64_t *n_best, bool out_device, int64_t *stats) {
  FA_REQUIRE(p, FA_ERR_INVALID, "null best-hit parameters");
  FA_REQUIRE(p->fragment_length >= 1, FA_ERR_INVALID, "fragment_length must be strictly positive");
  FA_REQUIRE(p->k >= 1, FA_ERR_INVALID, "k must be at least 1");
  FA_REQUIRE(p->min_identity >= 0.0f, FA_ERR_INVALID, "min_identity must be a number that is not negative");          // (false for NaN)
  FA_REQUIRE(p->min_aligned_fraction >= 0.0f, FA_ERR_INVALID, "min_aligned_fraction must be a number that is not negative");
  FA_REQUIRE(n_queries >= 0 && n_references >= 0 && n_rows >= 0, FA_ERR_INVALID, "negative table size");
  FA_REQUIRE(n_rows == 0 || rows, FA_ERR_INVALID, "null rows");
  FA_REQUIRE((n_queries == 0 || query_lengths) && (n_references == 0 || reference_lengths), FA_ERR_INVALID, "null genome lengths");
  FA_REQUIRE(!best || cap >= 0, FA_ERR_INVALID, "negative capacity");
  FA_REQUIRE(n_rows <= (int64_t)INT32_MAX, FA_ERR_UNSUPPORTED, "a table of more than 2^31 - 1 rows");
  require_device();
  CallStream stream;
  hipStream_t st = stream.s;
  StatusBlock<BestStatus> d_status(st);
  DevBuf<fa_cgi_row> d_rows;
  DevBuf<uint64_t> d_len;
  DevBuf<unsigned long long> keys, keys_sorted;
  DevBuf<uint32_t> row_of, row_of_sorted;
  DevBuf<unsigned char> temp;
  DevBuf<int32_t> seg;
  DevBuf<int64_t> d_offsets;

  BestArgs a{};
  a.n_rows = n_rows; a.n_queries = n_queries; a.n_references = n_references;
  a.fragment_length = (unsigned long long)p->fragment_length; a.min_fraction = p->min_fraction;
  a.min_identity = p->min_identity; a.min_aligned_fraction = p->min_aligned_fraction;
  a.k = p->k; a.exclude_self = p->exclude_self != 0 ? 1 : 0;
  a.ref_bits = id_bits(n_references);
  a.status = d_status.p;
  seg.ensure((size_t)n_queries * 2);
  if (n_queries) FA_HIP(hipMemsetAsync(seg.p, 0, (size_t)n_queries * 2 * sizeof(int32_t), st));
  a.seg_start = seg.p; a.seg_end = seg.p + n_queries;
  d_offsets.ensure((size_t)n_queries + 1);
  a.offsets = d_offsets.p;
  const dim3 row_grid(ceil_div(n_rows, 256));
  if (n_rows) {
    a.rows = on_device(rows, rows_device, (size_t)n_rows, d_rows, st);
    d_len.ensure((size_t)n_queries + (size_t)n_references);
    if (n_queries) FA_HIP(hipMemcpyAsync(d_len.p, query_lengths, (size_t)n_queries * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (n_references)
      FA_HIP(hipMemcpyAsync(d_len.p + n_queries, reference_lengths, (size_t)n_references * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    a.query_length = d_len.p; a.reference_length = d_len.p + n_queries;
    keys.ensure((size_t)n_rows); keys_sorted.ensure((size_t)n_rows);
    row_of.ensure((size_t)n_rows); row_of_sorted.ensure((size_t)n_rows);
    hipLaunchKernelGGL(k_best_keys, row_grid, dim3(256), 0, st, a, keys.p, row_of.p);
    // first sort: the bits of r and of the largest q (rows with an id out of range land anywhere: the call fails on the flag)
    unsigned end_bit = a.ref_bits + id_bits(n_queries);
    with_temp(temp, [&](void *t, size_t &bytes) {
      return rocprim::radix_sort_pairs(t, bytes, keys.p, keys_sorted.p, row_of.p, row_of_sorted.p, (size_t)n_rows, 0u, end_bit, st);
    });
    a.keys = keys_sorted.p; a.row_of = row_of_sorted.p;
    hipLaunchKernelGGL(k_best_rank_keys, row_grid, dim3(256), 0, st, a, keys.p);
    // second sort: 32 bits of identity and the bits of n_queries itself -- under them the all-ones key of a row that does
    // not survive reads 2^bits - 1 >= n_queries, behind every query
    end_bit = 32u + bit_width_u64((unsigned long long)n_queries);
    with_temp(temp, [&](void *t, size_t &bytes) {
      return rocprim::radix_sort_pairs(t, bytes, keys.p, keys_sorted.p, row_of_sorted.p, row_of.p, (size_t)n_rows, 0u, end_bit, st);
    });
    a.keys = keys_sorted.p; a.row_of = row_of.p;
    hipLaunchKernelGGL(k_best_segments, row_grid, dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(k_best_scan, dim3(1), dim3(1024), 0, st, a);
  FA_HIP(hipGetLastError());
  const BestStatus status = d_status.read(st);
  FA_REQUIRE(!(status.flags & TAB_BAD_ID), FA_ERR_INVALID, "a row names a query outside [0, n_queries) or a reference outside [0, n_references)");
  FA_REQUIRE(!(status.flags & TAB_DUPLICATE), FA_ERR_INVALID, "the table holds the same (query, reference) twice");
  const int64_t n_records = (int64_t)status.records;
  if (n_best) *n_best = n_records;
  FA_REQUIRE(!best || n_records <= cap, FA_ERR_INVALID, "the record buffer is smaller than the number of records");
  Staged<fa_cgi_row> records(best, out_device, (size_t)n_records);
  if (best && n_records) {
    a.best = reinterpret_cast<int32_t *>(records.dev());
    hipLaunchKernelGGL(k_best_write, row_grid, dim3(256), 0, st, a);
    FA_HIP(hipGetLastError());
    records.finish(st);
  }
  if (offsets)
    FA_HIP(hipMemcpyAsync(offsets, d_offsets.p, ((size_t)n_queries + 1) * sizeof(int64_t),
                          out_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  FA_HIP(hipStreamSynchronize(st));
  if (stats) { stats[0] = (int64_t)status.survivors; stats[1] = (int64_t)status.queries; stats[2] = n_records; }
}

// ------------------------------------------------------------------------------------------------------------
// The genome-level screen: bottom-s signatures, their pairs above a Jaccard cut-off, the groups (fa_screen.hip.h)
// ------------------------------------------------------------------------------------------------------------
inline void screen_signatures(const uint32_t *d_hash, const int32_t *d_seq_id, int64_t n_records, const int32_t *sbf, int32_t n_genomes,
                              int32_t s, uint32_t *d_sig, int32_t *d_count) {
  FA_REQUIRE(s >= 1 && s <= SCR_MAX_S, FA_ERR_INVALID, "the signature size must be in [1, 4096]");
  FA_REQUIRE(n_genomes >= 0 && n_records >= 0, FA_ERR_INVALID, "negative number of genomes or records");
  FA_REQUIRE(n_records == 0 || (d_hash && d_seq_id), FA_ERR_INVALID, "null records");
  FA_REQUIRE(n_genomes == 0 || (sbf && d_sig && d_count), FA_ERR_INVALID, "null sequencesByFileInfo or null outputs");
  FA_REQUIRE(n_records == 0 || n_genomes > 0, FA_ERR_INVALID, "records without a genome");
  FA_REQUIRE(n_records <= (int64_t)INT32_MAX, FA_ERR_UNSUPPORTED, "more than 2^31 - 1 records");
  for (int32_t g = 0; g < n_genomes; g++)
    FA_REQUIRE(sbf[g] >= (g ? sbf[g - 1] : 0), FA_ERR_INVALID, "sequencesByFileInfo must not decrease");
  require_device();
  if (!n_genomes) return;
  CallStream stream;
  hipStream_t st = stream.s;
  StatusBlock<TableStatus> d_status(st);
  DevBuf<int32_t> d_sbf;
  DevBuf<unsigned long long> keys, keys_sorted;
  DevBuf<uint32_t> heads, rank, segs;
  DevBuf<unsigned char> temp;

  SigArgs a{};
  a.hash = d_hash; a.seq_id = d_seq_id; a.n_records = n_records; a.n_genomes = n_genomes; a.s = s;
  a.n_contigs = sbf[n_genomes - 1];
  a.sig = d_sig; a.count = d_count; a.status = d_status.p;
  const dim3 rec_grid(ceil_div(n_records, 256));
  if (n_records) {
    // the verdict on the records is read before an output is touched
    hipLaunchKernelGGL(k_sig_check, rec_grid, dim3(256), 0, st, a);
    FA_HIP(hipGetLastError());
    const TableStatus status = d_status.read(st);
    FA_REQUIRE(!(status.flags & TAB_BAD_ID), FA_ERR_INVALID, "a record's contig id lies outside [0, sequencesByFileInfo[n_genomes - 1])");
    FA_REQUIRE(!(status.flags & SCR_NOT_ASCENDING), FA_ERR_INVALID, "the records are not sorted by contig id");
  }
  segs.ensure((size_t)n_genomes * 2);
  FA_HIP(hipMemsetAsync(segs.p, 0, (size_t)n_genomes * 2 * sizeof(uint32_t), st));
  a.first = segs.p; a.last = segs.p + n_genomes;
  FA_HIP(hipMemsetAsync(d_sig, 0, (size_t)n_genomes * (size_t)s * sizeof(uint32_t), st));
  if (n_records) {
    d_sbf.upload(sbf, (size_t)n_genomes, st);
    a.sbf = d_sbf.p;
    keys.ensure((size_t)n_records); keys_sorted.ensure((size_t)n_records);
    heads.ensure((size_t)n_records); rank.ensure((size_t)n_records);
    hipLaunchKernelGGL(k_sig_keys<false>, rec_grid, dim3(256), 0, st, a, keys.p);
    // the bits a key can have set: 32 of the hash and those of the largest genome number
    const unsigned end_bit = 32u + id_bits(n_genomes);
    with_temp(temp, [&](void *t, size_t &bytes) {
      return rocprim::radix_sort_keys(t, bytes, keys.p, keys_sorted.p, (size_t)n_records, 0u, end_bit, st);
    });
    a.keys = keys_sorted.p;
    hipLaunchKernelGGL(k_sig_heads, rec_grid, dim3(256), 0, st, a, heads.p);
    with_temp(temp, [&](void *t, size_t &bytes) {
      return rocprim::exclusive_scan(t, bytes, heads.p, rank.p, 0u, (size_t)n_records, rocprim::plus<uint32_t>(), st);
    });
    a.rank = rank.p;
    hipLaunchKernelGGL(k_sig_segments, rec_grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_sig_write, rec_grid, dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(k_sig_counts, dim3(ceil_div(n_genomes, 256)), dim3(256), 0, st, a);
  FA_HIP(hipGetLastError());
  FA_HIP(hipStreamSynchronize(st));
}

inline void screen_pairs(const uint32_t *d_sig_a, const int32_t *d_count_a, int32_t n_a, const uint32_t *d_sig_b, const int32_t *d_count_b,
                         int32_t n_b, int32_t s, bool triangular, int32_t jn, int32_t jd, fa_screen_pair *pairs, int64_t cap,
                         int64_t *n_pairs, bool pairs_device, int64_t *stats) {
  FA_REQUIRE(s >= 1 && s <= SCR_MAX_S, FA_ERR_INVALID, "the signature size must be in [1, 4096]");
  FA_REQUIRE(jd >= 1 && jn >= 0 && jn <= jd, FA_ERR_INVALID, "the Jaccard cut-off needs 0 <= jn <= jd and jd >= 1");
  FA_REQUIRE(n_a >= 0 && n_b >= 0, FA_ERR_INVALID, "negative number of genomes");
  FA_REQUIRE((n_a == 0 || (d_sig_a && d_count_a)) && (n_b == 0 || (d_sig_b && d_count_b)), FA_ERR_INVALID, "null signatures");
  FA_REQUIRE(!triangular || (d_sig_a == d_sig_b && d_count_a == d_count_b && n_a == n_b), FA_ERR_INVALID,
             "the triangular mode takes one signature set: the same pointers and n_a == n_b");
  FA_REQUIRE(!pairs || cap >= 0, FA_ERR_INVALID, "negative capacity");
  require_device();
  CallStream stream;
  hipStream_t st = stream.s;
  StatusBlock<TableStatus> d_status(st);
  DevBuf<unsigned long long> mask;
  DevBuf<int32_t> chunk_count;
  DevBuf<int64_t> chunk_off;

  ScreenArgs a{};
  a.sig_a = d_sig_a; a.sig_b = d_sig_b; a.count_a = d_count_a; a.count_b = d_count_b;
  a.n_a = n_a; a.n_b = n_b; a.s = s; a.triangular = triangular ? 1 : 0; a.jn = jn; a.jd = jd;
  a.tile = screen_tile(s);
  a.tile_shift = (int32_t)bit_width_u64((unsigned long long)a.tile) - 1;
  a.tiles_a = ceil_div(n_a, a.tile);
  a.words_per_row = ((int64_t)n_b + 63) / 64;
  a.n_words = (int64_t)n_a * a.words_per_row;
  a.status = d_status.p;
  const int64_t n_chunks = (a.n_words + SCR_CHUNK - 1) / SCR_CHUNK;
  FA_REQUIRE(n_chunks <= (int64_t)INT32_MAX, FA_ERR_UNSUPPORTED, "a screen of more than 2^43 pairs");
  a.n_chunks = (int32_t)n_chunks;
  TableStatus status{};
  if (a.n_words) {
    mask.ensure((size_t)a.n_words);
    FA_HIP(hipMemsetAsync(mask.p, 0, (size_t)a.n_words * sizeof(unsigned long long), st));
    a.mask = mask.p;
    chunk_count.ensure((size_t)a.n_chunks); chunk_off.ensure((size_t)a.n_chunks);
    a.chunk_count = chunk_count.p; a.chunk_off = chunk_off.p;
    const dim3 grid((unsigned)ceil_div(n_b, a.tile), (unsigned)std::min(a.tiles_a, 65535));
    // elements of A a lane searches at a time (measured at s = 64, 1000 and 4096, profiles/screen_pair_kernel.txt): a signature
    // of one pass gains nothing from a second chain, long ones hide more of the reads' latency behind more chains
    const size_t lds = (size_t)2 * a.tile * screen_stride(s) * sizeof(uint32_t);
    if (s <= 64) hipLaunchKernelGGL(k_screen_pairs<1>, grid, dim3(SCR_THREADS), lds, st, a);
    else if (s <= 2048) hipLaunchKernelGGL(k_screen_pairs<2>, grid, dim3(SCR_THREADS), lds, st, a);
    else hipLaunchKernelGGL(k_screen_pairs<4>, grid, dim3(SCR_THREADS), lds, st, a);
    hipLaunchKernelGGL(k_screen_count, dim3(ceil_div(a.n_chunks, 4)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_chunk_scan, dim3(1), dim3(1024), 0, st, a.chunk_count, a.chunk_off, a.n_chunks, &d_status.p->emitted);
    FA_HIP(hipGetLastError());
    status = d_status.read(st);
    FA_REQUIRE(!(status.flags & SCR_BAD_COUNT), FA_ERR_INVALID, "a signature count lies outside [0, s]");
    FA_REQUIRE(!(status.flags & SCR_NOT_ASCENDING), FA_ERR_INVALID, "a signature does not ascend strictly below its count");
  }
  const int64_t n_emit = (int64_t)status.emitted;
  if (n_pairs) *n_pairs = n_emit;
  FA_REQUIRE(!pairs || n_emit <= cap, FA_ERR_INVALID, "the pair buffer is smaller than the number of pairs");
  if (pairs && n_emit) {
    Staged<fa_screen_pair> out(pairs, pairs_device, (size_t)n_emit);
    a.pairs = out.dev();
    hipLaunchKernelGGL(k_screen_write, dim3(ceil_div(a.n_chunks, 4)), dim3(256), 0, st, a);
    FA_HIP(hipGetLastError());
    out.finish(st);
    FA_HIP(hipStreamSynchronize(st));
  }
  if (stats) {
    stats[0] = triangular ? (int64_t)n_a * ((int64_t)n_a - 1) / 2 : (int64_t)n_a * (int64_t)n_b;
    stats[1] = n_emit;
  }
}

inline void screen_groups(const fa_screen_pair *pairs, int64_t n_pairs, bool pairs_device, int32_t n_genomes, int32_t *labels,
                          bool labels_device, int32_t *n_groups) {
  FA_REQUIRE(n_genomes >= 0 && n_pairs >= 0, FA_ERR_INVALID, "negative number of genomes or pairs");
  FA_REQUIRE(n_pairs == 0 || pairs, FA_ERR_INVALID, "null pairs");
  FA_REQUIRE(n_genomes == 0 || labels, FA_ERR_INVALID, "null labels");
  FA_REQUIRE(n_pairs <= (int64_t)INT32_MAX, FA_ERR_UNSUPPORTED, "more than 2^31 - 1 pairs");
  require_device();
  CallStream stream;
  hipStream_t st = stream.s;
  StatusBlock<TableStatus> d_status(st);
  DevBuf<fa_screen_pair> d_pairs;
  DevBuf<int2> d_edges;
  if (n_pairs) {
    pairs = on_device(pairs, pairs_device, (size_t)n_pairs, d_pairs, st);
    d_edges.ensure((size_t)n_pairs);
    hipLaunchKernelGGL(k_screen_edges, dim3(ceil_div(n_pairs, 256)), dim3(256), 0, st, pairs, n_pairs, n_genomes, d_edges.p, d_status.p);
    FA_HIP(hipGetLastError());
    const TableStatus status = d_status.read(st);
    FA_REQUIRE(!(status.flags & TAB_BAD_ID), FA_ERR_INVALID, "a pair is not 0 <= a < b < n_genomes");
  }
  unsigned int roots = 0;
  if (n_genomes) {
    Staged<int32_t> out(labels, labels_device, (size_t)n_genomes);
    int64_t rounds = 0;
    roots = components(d_edges.p, n_pairs, out.dev(), n_genomes, d_status.p, st, rounds);
    out.finish(st);
    FA_HIP(hipStreamSynchronize(st));
  }
  if (n_groups) *n_groups = (int32_t)roots;
}

// ------------------------------------------------------------------------------------------------------------
// The containment road of the screen: a collection's contents as a sorted directory, signatures looked up in it
// (fa_contain.hip.h has the semantics and the road)
// ------------------------------------------------------------------------------------------------------------
inline void screen_contents(const uint32_t *d_hash, const int32_t *d_seq_id, int64_t n_records, const int32_t *sbf, int32_t n_genomes,
                            uint32_t *d_ent_hash, int32_t *d_ent_genome, int64_t cap, int64_t *n_entries) {
  FA_REQUIRE(n_genomes >= 0 && n_records >= 0, FA_ERR_INVALID, "negative number of genomes or records");
  FA_REQUIRE(n_records == 0 || (d_hash && d_seq_id), FA_ERR_INVALID, "null records");
  FA_REQUIRE(n_genomes == 0 || sbf, FA_ERR_INVALID, "null sequencesByFileInfo");
  FA_REQUIRE(n_records == 0 || n_genomes > 0, FA_ERR_INVALID, "records without a genome");
  FA_REQUIRE((d_ent_hash == nullptr) == (d_ent_genome == nullptr), FA_ERR_INVALID, "the entries' hashes and genomes come together or not at all");
  FA_REQUIRE(!d_ent_hash || cap >= 0, FA_ERR_INVALID, "negative capacity");
  FA_REQUIRE(n_records <= (int64_t)INT32_MAX, FA_ERR_UNSUPPORTED, "more than 2^31 - 1 records");
  for (int32_t g = 0; g < n_genomes; g++)
    FA_REQUIRE(sbf[g] >= (g ? sbf[g - 1] : 0), FA_ERR_INVALID, "sequencesByFileInfo must not decrease");
  require_device();
  if (!n_records) {
    if (n_entries) *n_entries = 0;
    return;
  }
  CallStream stream;
  hipStream_t st = stream.s;
  StatusBlock<TableStatus> d_status(st);
  DevBuf<int32_t> d_sbf;
  DevBuf<unsigned long long> keys, keys_sorted;
  DevBuf<uint32_t> heads;
  DevBuf<unsigned char> temp;
  DevBuf<int32_t> chunk_count;
  DevBuf<int64_t> chunk_off;

  SigArgs a{};
  a.hash = d_hash; a.seq_id = d_seq_id; a.n_records = n_records; a.n_genomes = n_genomes;
  a.n_contigs = sbf[n_genomes - 1];
  a.status = d_status.p;
  const dim3 rec_grid(ceil_div(n_records, 256));
  // the verdict on the records is read before anything else runs
  hipLaunchKernelGGL(k_sig_check, rec_grid, dim3(256), 0, st, a);
  FA_HIP(hipGetLastError());
  TableStatus status = d_status.read(st);
  FA_REQUIRE(!(status.flags & TAB_BAD_ID), FA_ERR_INVALID, "a record's contig id lies outside [0, sequencesByFileInfo[n_genomes - 1])");
  FA_REQUIRE(!(status.flags & SCR_NOT_ASCENDING), FA_ERR_INVALID, "the records are not sorted by contig id");
  d_sbf.upload(sbf, (size_t)n_genomes, st);
  a.sbf = d_sbf.p;
  keys.ensure((size_t)n_records); keys_sorted.ensure((size_t)n_records);
  heads.ensure((size_t)n_records);
  // the bits a key can have set: those of the largest genome number and 32 of the hash above them
  a.genome_bits = (int32_t)id_bits(n_genomes);
  const unsigned end_bit = 32u + (unsigned)a.genome_bits;
  hipLaunchKernelGGL(k_sig_keys<true>, rec_grid, dim3(256), 0, st, a, keys.p);
  with_temp(temp, [&](void *t, size_t &bytes) {
    return rocprim::radix_sort_keys(t, bytes, keys.p, keys_sorted.p, (size_t)n_records, 0u, end_bit, st);
  });
  a.keys = keys_sorted.p;
  hipLaunchKernelGGL(k_sig_heads, rec_grid, dim3(256), 0, st, a, heads.p);
  EntArgs e{};
  e.keys = keys_sorted.p; e.heads = heads.p; e.n_records = n_records;
  e.n_chunks = ceil_div(n_records, ENT_CHUNK); e.genome_bits = a.genome_bits;
  chunk_count.ensure((size_t)e.n_chunks); chunk_off.ensure((size_t)e.n_chunks);
  e.chunk_count = chunk_count.p; e.chunk_off = chunk_off.p;
  hipLaunchKernelGGL(k_ent_count, dim3(ceil_div(e.n_chunks, 4)), dim3(256), 0, st, e);
  hipLaunchKernelGGL(k_chunk_scan, dim3(1), dim3(1024), 0, st, e.chunk_count, e.chunk_off, e.n_chunks, &d_status.p->emitted);
  FA_HIP(hipGetLastError());
  status = d_status.read(st);
  const int64_t m = (int64_t)status.emitted;
  if (n_entries) *n_entries = m;
  if (!d_ent_hash) return;
  FA_REQUIRE(m <= cap, FA_ERR_INVALID, "the entry buffers are smaller than the number of entries");
  e.ent_hash = d_ent_hash; e.ent_genome = d_ent_genome;
  hipLaunchKernelGGL(k_ent_write, dim3(ceil_div(e.n_chunks, 4)), dim3(256), 0, st, e);
  FA_HIP(hipGetLastError());
  FA_HIP(hipStreamSynchronize(st));
}

// the threads of a k_contain_winner workgroup, 512 or 1024: WIN_THREADS unless fa_debug_contain_winner_threads has set the other
inline std::atomic<int> g_winner_threads{WIN_THREADS};

// fa_screen_contained, and with `winner` fa_screen_contained_winner (d_weight: its optional weights): the same call but for the
// statistic the records carry -- the elements a reference holds, or those it wins
inline void screen_contained(const uint32_t *d_sig, const int32_t *d_count, int32_t n_a, int32_t s, const uint32_t *d_ent_hash,
                             const int32_t *d_ent_genome, int64_t n_entries, int32_t n_b, bool winner, const int32_t *d_weight, int32_t cn,
                             int32_t cd, fa_screen_pair *pairs, int64_t cap, int64_t *n_pairs, bool pairs_device, int64_t *stats) {
  FA_REQUIRE(s >= 1 && s <= SCR_MAX_S, FA_ERR_INVALID, "the signature size must be in [1, 4096]");
  FA_REQUIRE(cd >= 1 && cn >= 0 && cn <= cd, FA_ERR_INVALID, "the containment cut-off needs 0 <= cn <= cd and cd >= 1");
  FA_REQUIRE(n_a >= 0 && n_b >= 0 && n_entries >= 0, FA_ERR_INVALID, "negative number of genomes or entries");
  FA_REQUIRE(n_a == 0 || (d_sig && d_count), FA_ERR_INVALID, "null signatures");
  FA_REQUIRE(n_entries == 0 || (d_ent_hash && d_ent_genome), FA_ERR_INVALID, "null entries");
  FA_REQUIRE(!pairs || cap >= 0, FA_ERR_INVALID, "negative capacity");
  const int64_t n_slices = std::max<int64_t>(1, ((int64_t)n_b + CNT_SLICE - 1) / CNT_SLICE);
  const int64_t n_groups = (int64_t)n_a * n_slices;
  FA_REQUIRE(n_groups <= (int64_t)INT32_MAX, FA_ERR_UNSUPPORTED, "more than 2^31 - 1 (query, slice of references) workgroups");
  require_device();
  CallStream stream;
  hipStream_t st = stream.s;
  StatusBlock<ContainStatus> d_status(st);
  DevBuf<int32_t> group_count;
  DevBuf<int64_t> group_off;
  DevBuf<int32_t> winners;

  ContainArgs a{};
  a.weight = winner ? d_weight : nullptr;
  a.sig = d_sig; a.count = d_count; a.n_a = n_a; a.s = s;
  a.ent_hash = d_ent_hash; a.ent_genome = d_ent_genome; a.m = n_entries; a.n_b = n_b; a.n_slices = (int32_t)n_slices;
  a.cn = cn; a.cd = cd; a.status = d_status.p;
  ContainStatus status{};
  const int64_t to_check = std::max({(int64_t)n_a * s, n_entries, a.weight ? (int64_t)n_b : (int64_t)0});
  if (to_check) {
    // the verdict on both inputs is read before a counting kernel is launched: those rely on it
    hipLaunchKernelGGL(k_contain_check, dim3((unsigned)std::min<int64_t>((to_check + 255) / 256, 1 << 20)), dim3(256), 0, st, a);
    FA_HIP(hipGetLastError());
    status = d_status.read(st);
    FA_REQUIRE(!(status.flags & SCR_BAD_COUNT), FA_ERR_INVALID, "a signature count lies outside [0, s]");
    FA_REQUIRE(!(status.flags & SCR_NOT_ASCENDING), FA_ERR_INVALID, "a signature does not ascend strictly below its count");
    FA_REQUIRE(!(status.flags & TAB_BAD_ID), FA_ERR_INVALID, "an entry names a genome outside [0, n_b)");
    FA_REQUIRE(!(status.flags & CNT_UNORDERED), FA_ERR_INVALID, "the entries do not ascend strictly by (hash, genome)");
    FA_REQUIRE(!(status.flags & CNT_BAD_WEIGHT), FA_ERR_INVALID, "a weight is negative");
  }
  // the COUNT or the WRITE form; elements of A a thread searches at a time: as many chains as a signature of size s gives a
  // thread of CNT_THREADS, four at the most (not measured yet: scripts/time_contain.py)
  const size_t lds = (size_t)((std::min<int64_t>(n_b, CNT_SLICE) + 1) / 2) * sizeof(uint32_t);
  auto launch = [&](bool write) {
    const dim3 grid((unsigned)n_groups), block(CNT_THREADS);
    if (winner) {
      if (write) hipLaunchKernelGGL(k_contain_won<true>, grid, block, lds, st, a);
      else hipLaunchKernelGGL(k_contain_won<false>, grid, block, lds, st, a);
    } else if (s <= CNT_THREADS) {
      if (write) hipLaunchKernelGGL((k_contain<1, true>), grid, block, lds, st, a);
      else hipLaunchKernelGGL((k_contain<1, false>), grid, block, lds, st, a);
    } else if (s <= 2 * CNT_THREADS) {
      if (write) hipLaunchKernelGGL((k_contain<2, true>), grid, block, lds, st, a);
      else hipLaunchKernelGGL((k_contain<2, false>), grid, block, lds, st, a);
    } else {
      if (write) hipLaunchKernelGGL((k_contain<4, true>), grid, block, lds, st, a);
      else hipLaunchKernelGGL((k_contain<4, false>), grid, block, lds, st, a);
    }
  };
  if (n_a && n_b) {
    group_count.ensure((size_t)n_groups); group_off.ensure((size_t)n_groups);
    a.group_count = group_count.p; a.group_off = group_off.p;
    if (winner) {
      // every element's winner, once for both forms: one workgroup per query, the slices' counters and 20 bytes per element
      // of the signature in LDS -- beyond 64 KiB for a large collection, one workgroup per CU either way
      winners.ensure((size_t)n_a * (size_t)s);
      a.winner = winners.p;
      const size_t lds_w = lds + (size_t)s * 20;
      const int threads = g_winner_threads.load();
      auto go = [&](auto kernel) {
        if (lds_w > 64 * 1024) FA_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_w));
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_a), dim3((unsigned)threads), lds_w, st, a);
      };
      const int chains = (s + threads - 1) / threads;                 // searches a thread has in flight, four at the most
      if (threads == 512) {
        if (chains <= 1) go(k_contain_winner<512, 1>);
        else if (chains <= 2) go(k_contain_winner<512, 2>);
        else go(k_contain_winner<512, 4>);
      } else {
        if (chains <= 1) go(k_contain_winner<1024, 1>);
        else if (chains <= 2) go(k_contain_winner<1024, 2>);
        else go(k_contain_winner<1024, 4>);
      }
    }
    launch(false);
    hipLaunchKernelGGL(k_chunk_scan, dim3(1), dim3(1024), 0, st, a.group_count, a.group_off, (int32_t)n_groups, &d_status.p->emitted);
    FA_HIP(hipGetLastError());
    status = d_status.read(st);
  }
  const int64_t n_emit = status.emitted;
  if (n_pairs) *n_pairs = n_emit;
  FA_REQUIRE(!pairs || n_emit <= cap, FA_ERR_INVALID, "the pair buffer is smaller than the number of pairs");
  if (pairs && n_emit) {
    Staged<fa_screen_pair> out(pairs, pairs_device, (size_t)n_emit);
    a.pairs = out.dev();
    launch(true);
    FA_HIP(hipGetLastError());
    out.finish(st);
    FA_HIP(hipStreamSynchronize(st));
  }
  if (stats) {
    stats[0] = (int64_t)n_a * (int64_t)n_b;
    stats[1] = n_emit;
    stats[2] = (int64_t)status.visited;
    if (winner) stats[3] = (int64_t)status.assigned;
  }
}

// ------------------------------------------------------------------------------------------------------------
// The bottom-s signatures of a resident batch, pass by pass (fa_batchsig.hip.h has the semantics and the road)
// ------------------------------------------------------------------------------------------------------------
// The call is not a query: the workspace it borrows becomes the lease's "most recent" one when it is handed back, and this
// puts the mapper's own choice back behind it, so that timings, kernel forms and stage getters go on speaking of the last
// query.  (Declared before the lease: destroyed after it.  A query that another thread finishes while the call runs loses
// its place to the one before it: "most recent" is a single-caller notion, as it is between two concurrent queries.)
struct KeepLastWorkspace {
  fa_mapper &m;
  int ws;
  explicit KeepLastWorkspace(fa_mapper &mm) : m(mm) { std::lock_guard<std::mutex> lock(m.mtx); ws = m.last_ws; }
  ~KeepLastWorkspace() { std::lock_guard<std::mutex> lock(m.mtx); m.last_ws = ws; }
};

// Of a workspace only K1's staging arrays (Workspace::sk) are written -- no stage getter reads them, every pass of a query
// fills them anew -- so what the getters return after the call is what they returned before it.
inline void genomes_signatures(fa_mapper *m, fa_genomes *g, int32_t first, int32_t count, int32_t s, int64_t pass_frags, uint32_t *d_sig,
                               int32_t *d_count, int64_t *stats) {
  FA_REQUIRE(m && g, FA_ERR_INVALID, "null mapper or batch");
  FA_REQUIRE(s >= 1 && s <= SCR_MAX_S, FA_ERR_INVALID, "the signature size must be in [1, 4096]");
  FA_REQUIRE(first >= 0 && count >= 0 && (int64_t)first + (int64_t)count <= (int64_t)g->n_genomes, FA_ERR_INVALID, "genome range out of bounds");
  FA_REQUIRE(pass_frags >= 0, FA_ERR_INVALID, "negative number of fragments per pass");
  FA_REQUIRE(count == 0 || (d_sig && d_count), FA_ERR_INVALID, "null outputs");
  FA_REQUIRE(g->P.kmer_size == m->P.kmer_size && g->P.window_size == m->P.window_size && g->P.fragment_length == m->P.fragment_length &&
                 g->P.alphabet_size == m->P.alphabet_size, FA_ERR_INVALID, "the batch was uploaded with other parameters than the mapper's");
  require_device();
  const int64_t per_pass = pass_frags ? pass_frags : pass_fragments();
  const std::vector<int64_t> &lo = g->genome_frag_lo;
  const int64_t F0 = count ? lo[(size_t)first] : 0, F1 = count ? lo[(size_t)first + (size_t)count] : 0;
  int64_t passes = 0;
  double k1_ms = 0, all_ms = 0;
  if (count) {
    KeepLastWorkspace keep(*m);
    WorkspaceLease lease(*m);
    Workspace &w = *lease.w;
    hipStream_t st = w.stream;
    bool timed;
    { std::lock_guard<std::mutex> lock(m->mtx); timed = m->stage_events; }
    std::vector<Event> ev;                               // three a pass: its begin, behind K1, its end
    DevBuf<uint32_t> carry, heads, rank, segs;
    DevBuf<int32_t> tile_off;
    DevBuf<unsigned long long> keys, sorted;
    DevBuf<unsigned char> temp;
    carry.ensure((size_t)s + 1);
    FA_HIP(hipMemsetAsync(d_sig, 0, (size_t)count * (size_t)s * sizeof(uint32_t), st));
    FA_HIP(hipMemsetAsync(d_count, 0, (size_t)count * sizeof(int32_t), st));
    // the genome that holds fragment f (genomes without fragments hold none)
    auto genome_of = [&](int64_t f) { return (int32_t)(std::upper_bound(lo.begin(), lo.end(), f) - lo.begin()) - 1; };
    auto mark = [&] { if (timed) { ev.emplace_back(); FA_HIP(hipEventRecord(ev.back().get(), st)); } };
    for (int64_t f0 = F0, f1; f0 < F1; f0 = f1, passes++) {
      f1 = std::min(F1, f0 + per_pass);
      const int32_t t0 = g->frag_tile_lo[(size_t)f0], ntiles = g->frag_tile_lo[(size_t)f1] - t0;
      const int32_t g0 = genome_of(f0), g1 = genome_of(f1 - 1);
      const bool carried = f0 > lo[(size_t)g0], goes_on = lo[(size_t)g1 + 1] > f1;
      BatchSigArgs a{};
      a.tiles = g->tiles + t0; a.ntiles = ntiles; a.frag_query = g->d_frag_query; a.f0 = f0; a.f1 = f1;
      a.g0 = g0; a.n_genomes = g1 - g0 + 1; a.cont = goes_on ? g1 - g0 : -1; a.s = s; a.carry = carry.p;
      a.sig = d_sig + (size_t)(g0 - first) * (size_t)s; a.count = d_count + (g0 - first);
      // (the scan below and the ranks of the heads are 32-bit: the slots of a pass and a carried signature stay within them)
      FA_REQUIRE((int64_t)ntiles * TILE + s <= (int64_t)INT32_MAX, FA_ERR_UNSUPPORTED, "more than 2^31 - 1 record slots in one pass: lower the fragments per pass");
      mark();
      w.sk.reserve((size_t)std::max(ntiles, 1));
      launch_sketch_tiles(m->P, g->store, a.tiles, ntiles, w.sk.stage_hash.p, w.sk.stage_wpos.p, w.sk.tile_count.p, st);
      mark();
      tile_off.ensure((size_t)ntiles + 1);
      FA_HIP(hipMemsetAsync(w.sk.tile_count.p + ntiles, 0, sizeof(int32_t), st));
      exclusive_sum_i32(temp, w.sk.tile_count.p, tile_off.p, (size_t)ntiles + 1, st);
      // the sizes of the pass: its staged records, and the carried partial signature of a genome that began before it
      int32_t n_staged = 0;
      uint32_t carry_in = 0;
      FA_HIP(hipMemcpyAsync(&n_staged, tile_off.p + ntiles, sizeof n_staged, hipMemcpyDeviceToHost, st));
      if (carried) FA_HIP(hipMemcpyAsync(&carry_in, carry.p + s, sizeof carry_in, hipMemcpyDeviceToHost, st));
      FA_HIP(hipStreamSynchronize(st));
      FA_REQUIRE(n_staged >= 0 && n_staged <= (int64_t)ntiles * TILE && carry_in <= (uint32_t)s, FA_ERR_INTERNAL, "a tile staged more records than it has slots");
      const int64_t n_keys = (int64_t)n_staged + (int64_t)carry_in;
      if (!n_keys) {                                     // (fragments without a record: every genome of the pass keeps count 0)
        if (goes_on) FA_HIP(hipMemsetAsync(carry.p + s, 0, sizeof(uint32_t), st));
        mark();
        continue;
      }
      keys.ensure((size_t)n_keys); sorted.ensure((size_t)n_keys); heads.ensure((size_t)n_keys); rank.ensure((size_t)n_keys);
      segs.ensure((size_t)a.n_genomes * 2);
      FA_HIP(hipMemsetAsync(segs.p, 0, (size_t)a.n_genomes * 2 * sizeof(uint32_t), st));
      a.tile_count = w.sk.tile_count.p; a.tile_off = tile_off.p; a.stage_hash = w.sk.stage_hash.p;
      a.n_staged = n_staged; a.n_keys = n_keys; a.keys = keys.p; a.carry_in = (int32_t)carry_in;
      hipLaunchKernelGGL(k_bsig_keys, dim3(ceil_div(ntiles, 4)), dim3(256), 0, st, a);
      if (carry_in) hipLaunchKernelGGL(k_bsig_carry, dim3(ceil_div(carry_in, 256)), dim3(256), 0, st, a);
      // the bits a key can have set: 32 of the hash and those of the pass's largest genome number
      const unsigned end_bit = 32u + id_bits(a.n_genomes);
      with_temp(temp, [&](void *t, size_t &bytes) {
        return rocprim::radix_sort_keys(t, bytes, keys.p, sorted.p, (size_t)n_keys, 0u, end_bit, st);
      });
      SigArgs sa{};                                      // the heads, their ranks and every genome's segment: fa_screen.hip.h's own
      sa.keys = sorted.p; sa.n_records = n_keys; sa.first = segs.p; sa.last = segs.p + a.n_genomes;
      const dim3 key_grid(ceil_div(n_keys, 256));
      hipLaunchKernelGGL(k_sig_heads, key_grid, dim3(256), 0, st, sa, heads.p);
      with_temp(temp, [&](void *t, size_t &bytes) {
        return rocprim::exclusive_scan(t, bytes, heads.p, rank.p, 0u, (size_t)n_keys, rocprim::plus<uint32_t>(), st);
      });
      sa.rank = rank.p;
      hipLaunchKernelGGL(k_sig_segments, key_grid, dim3(256), 0, st, sa);
      a.sorted = sorted.p; a.rank = rank.p; a.first = sa.first; a.last = sa.last;
      hipLaunchKernelGGL(k_bsig_write, key_grid, dim3(256), 0, st, a);
      hipLaunchKernelGGL(k_bsig_counts, dim3(ceil_div(a.n_genomes, 256)), dim3(256), 0, st, a);
      FA_HIP(hipGetLastError());
      mark();
    }
    FA_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i + 2 < ev.size(); i += 3) {
      float k1 = 0, all = 0;
      FA_HIP(hipEventElapsedTime(&k1, ev[i], ev[i + 1]));
      FA_HIP(hipEventElapsedTime(&all, ev[i], ev[i + 2]));
      k1_ms += k1; all_ms += all;
    }
  }
  if (stats) {
    stats[0] = F1 - F0; stats[1] = passes;
    stats[2] = (int64_t)std::llround(k1_ms * 1e3); stats[3] = (int64_t)std::llround(all_ms * 1e3);
  }
}

}  // namespace fa
