// fa_batchsig.hip.h -- the bottom-s signatures of a resident query batch (fa_genomes_signatures), made pass by pass in
// bounded memory: what fa_screen_signatures makes of a sketch's records, made of the fragments a batch already holds, so
// that queries are uploaded once, screened and mapped.  Nothing here is on the mapping path: the kernels run only under that
// entry point, on the stream of the workspace it borrows.
//
// Semantics.  The signature of genome g is taken from the query sketches of its fragments [genome_frag_lo[g],
// genome_frag_lo[g + 1]) -- the sets the mapper itself maps with (fa_mapper_debug_query_sketch).  With d_g the number of
// distinct hashes in their union, the signature is the min(s, d_g) smallest of them, ascending as unsigned 32-bit, count[g] =
// min(s, d_g), the entries from count[g] up to s are 0, and a genome without fragments has count 0.  Layout and range of s
// are those of fa_screen.hip.h.  A fragment's query sketch is the distinct hashes of the records K1 stages for its tiles
// (the leading-run rule of the per-fragment sketch only drops repeats of a hash that stays), so the union over a genome is
// the distinct staged hashes of its tiles.
//
// The road, per pass of at most `pass size` fragments (cut anywhere, not only at genome boundaries):
//   1. K1 (launch_sketch_tiles, every form it picks) fills the workspace's staging arrays for the pass's own tiles;
//   2. an exclusive scan of tile_count places every tile's records;
//   3. k_bsig_keys compacts the sparse staging (TILE slots a tile, about 2 / (w + 1) of them filled) into dense 64-bit keys
//      (genome - first genome of the pass) << 32 | hash, the genome being that of the tile's fragment (frag_query);
//   4. k_bsig_carry appends the partial signature of the genome that began in an earlier pass, as keys of genome 0;
//   5. one radix sort over 32 bits plus those of the pass's genome count;
//   6. heads, their scan and the segments are the kernels of fa_screen.hip.h (k_sig_heads, k_sig_segments);
//   7. k_bsig_write stores the first s heads of every genome that ends in the pass into sig, and those of the one genome that
//      goes on into the next pass into the carry buffer (s words and a count); k_bsig_counts does the same for the counts.
// The carry is exact because  bottom-s(A u B) = bottom-s(bottom-s(A) u B):  an element of the left side is among the s
// smallest of A u B, hence among the s smallest of A if it lies in A at all, so nothing the carry dropped could have been
// kept.  Keys and sort temporaries are sized by the records of ONE pass; nothing is sized by the batch.  No hash bound drops
// keys before the sort (profiles/EXPERIMENTS.md has the split between K1 and the rest).
#pragma once

#include "fa_screen.hip.h"
#include "fa_sketch.hip.h"

namespace fa {

struct BatchSigArgs {
  const Tile *tiles;                   // the pass's own tiles of the batch
  int32_t ntiles;
  const int32_t *tile_count;           // [ntiles] staged records of every tile
  const int32_t *tile_off;             // [ntiles + 1] their exclusive scan
  const uint32_t *stage_hash;          // [ntiles][TILE]
  const int32_t *frag_query;           // batch-wide: the genome of every fragment
  int64_t f0, f1;                      // the fragments of the pass
  int32_t g0, n_genomes;               // the first genome of the pass and how many it touches
  int64_t n_staged, n_keys;            // records of the pass; with the carried keys behind them
  unsigned long long *keys;            // [n_keys]
  uint32_t *carry;                     // [s + 1]: a partial signature and, in word s, its count
  int32_t carry_in;                    // carried keys of this pass (genome 0 of the pass)
  int32_t cont;                        // the pass-local genome that goes on into the next pass, or -1
  int32_t s;
  const unsigned long long *sorted;
  const uint32_t *rank;                // exclusive scan of the heads
  const uint32_t *first, *last;        // [n_genomes] head ranks of every genome of the pass (k_sig_segments)
  uint32_t *sig;                       // row 0 = genome g0
  int32_t *count;
};

// one wave per tile: its staged records, dense, under the genome of its fragment
__global__ __launch_bounds__(256) void k_bsig_keys(BatchSigArgs a) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= a.ntiles) return;                                          // (wave-uniform)
  const int64_t f = a.tiles[t].seq;
  if (f < a.f0 || f >= a.f1) return;
  const int32_t g = a.frag_query[f] - a.g0;
  if (g < 0 || g >= a.n_genomes) return;
  const int64_t off = a.tile_off[t];
  const int c = min(max(a.tile_count[t], 0), TILE);
  const unsigned long long hi = (unsigned long long)(uint32_t)g << 32;
  for (int i = lane; i < c; i += 64)
    if (off + i < a.n_staged) a.keys[off + i] = hi | a.stage_hash[(size_t)t * TILE + i];
}

__global__ __launch_bounds__(256) void k_bsig_carry(BatchSigArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.carry_in) a.keys[a.n_staged + i] = (unsigned long long)a.carry[i];
}

// k_sig_write with two destinations: the genome that goes on writes its heads into the carry buffer
__global__ __launch_bounds__(256) void k_bsig_write(BatchSigArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_keys) return;
  const unsigned long long key = a.sorted[i];
  if (i > 0 && a.sorted[i - 1] == key) return;
  const uint32_t g = (uint32_t)(key >> 32);
  const uint32_t r = a.rank[i] - a.first[g];
  if (r >= (uint32_t)a.s) return;
  if ((int32_t)g == a.cont) a.carry[r] = (uint32_t)key;
  else a.sig[(size_t)g * (size_t)a.s + r] = (uint32_t)key;
}

__global__ __launch_bounds__(256) void k_bsig_counts(BatchSigArgs a) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= a.n_genomes) return;
  const uint32_t c = min(a.last[g] - a.first[g], (uint32_t)a.s);
  if (g == a.cont) a.carry[a.s] = c;
  else a.count[g] = (int32_t)c;
}

}  // namespace fa
