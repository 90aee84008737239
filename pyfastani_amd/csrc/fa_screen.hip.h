// fa_screen.hip.h -- a genome-level screen on the device: every genome reduced to a bottom-s MinHash signature of its
// minimizer hashes (fa_screen_signatures), all pairs of one signature set or of two sets reduced to the pairs above a Jaccard
// cut-off with their shared and union counts (fa_screen_pairs), and the connected groups of such pairs (fa_screen_groups,
// through the component loop of fa_table.hip.h).  Nothing here is on the mapping path: the kernels run only under those
// three entry points, on a stream of the call's own.
//
// Semantics
//   1. Signature.  Genome g owns the records whose contig id lies in [sbf[g-1], sbf[g]) (sbf = sequencesByFileInfo, sbf[-1] =
//      0); records are sorted by contig id.  With d_g the number of distinct hash values of g's records, the signature of g
//      is the min(s, d_g) smallest of them, ascending as unsigned 32-bit, and count[g] = min(s, d_g); a genome without
//      records has count 0.  Layout: uint32 sig[n_genomes][s], int32 count[n_genomes]; the entries from count[g] up to s are
//      0.  The count delimits a signature, not a sentinel: 0 and 0xFFFFFFFF are both legal hashes.  1 <= s <= 4096.
//      This is the bottom-s sketch of the genome's WINNOWED minimizers, not of all its k-mers.  A k-mer whose hash is among
//      a contig's smallest is almost always some window's minimum, so the two sketches nearly coincide; the claim is
//      "Mash-like at the sketch's k", not equality with the Mash program.
//   2. Pair statistic (Mash's merge rule).  For signatures A and B made with the same s, let U be their ascending distinct
//      union; denom = min(s, |U|); shared = the number of the first denom elements of U that occur in both.  denom == 0
//      (two empty genomes) never forms a pair.
//   3. Pair filter.  A pair is kept iff denom > 0 and (int64)shared * jd >= (int64)jn * denom, jn / jd being the caller's
//      rational Jaccard cut-off, 0 <= jn <= jd, jd >= 1, both int32: integers only, so no two implementations can disagree
//      at a boundary.
//   4. Output.  fa_screen_pair { int32 a, b, shared, denom } sorted by (a, b).  Triangular: one set, the pairs a < b.
//      Rectangular: two sets, every (a, b), a indexing the first and b the second.  The same input gives the same bytes on
//      every run.
//   5. Groups.  The connected components of triangular pair records: labels[g] = the smallest genome number of g's group.
//
// Signatures.  k_sig_check raises a flag for a contig id that descends or lies outside [0, sbf[n_genomes-1]) -- the host
// reads it before anything is written.  k_sig_keys finds every record's genome by binary search in sbf and packs
// genome << 32 | hash (its other form packs the hash above the genome: the contents of fa_contain.hip.h); one radix sort
// over 32 bits plus those of the largest genome number orders every genome's hashes; a head is a key that differs from
// its predecessor; an exclusive scan of the heads ranks them, the rank of a genome's first key (always a head) is the base
// of its segment (k_sig_segments: the one thread that sees a boundary writes it), and k_sig_write stores the heads of
// segment rank below s.
//
// Pairs, the hot path.  A workgroup of SCR_WAVES waves owns a tile of T x T genomes and stages the 2 T signatures once in
// LDS, checking on the way that counts lie in [0, s] and signatures ascend strictly.  A row of LDS is screen_stride(s) words,
// the power of two that holds s, and T = screen_tile(s) is the largest power of two <= 64 with 2 T rows within SCR_LDS_WORDS,
// so small s takes more genomes per tile.  A wave evaluates one pair at a time with no sequential merge: lane l takes the
// elements l, l + 64, ... of A; a branch-free binary search over B's row gives the element's lower bound and whether it
// occurs in B -- the B rows are filled with 0xFFFFFFFF behind their count, so a step of the search is an address, a read,
// a compare and a select, with no test against |B|; with m the matches before the element -- a running total plus the
// population count of the ballot below the lane -- its rank in the distinct union is  position + lower bound - m; the wave
// adds up the matches of rank below s.  Ranks ascend with the position, so the pass over A ends as soon as a rank reaches s
// (then |U| > s and denom = s); otherwise the total number of matches gives |U| = |A| + |B| - matches.  A lane searches E
// elements at a time, their reads issued together (E is the engine's choice by s; profiles/EXPERIMENTS.md has the
// measurements).  A kept pair sets bit b of row a in a bit mask of n_a x n_b (atomicOr: the outcome does not depend on
// order).  The pairs then come out in (a, b) order by count / scan / write over chunks of SCR_CHUNK mask words (the form of
// k_table_count / k_chunk_scan / k_table_write, the scan being the same kernel): a chunk's wave walks its set bits in order
// and evaluates each kept pair again, straight from global memory, for its two counts -- the mask costs one bit per pair
// where the statistics would cost eight bytes, and kept pairs are few where a screen is of use.  No atomic decides a
// record's place.
#pragma once

#include "fa_table.hip.h"

namespace fa {

constexpr int SCR_MAX_S = 4096;
constexpr int SCR_WAVES = 8, SCR_THREADS = 64 * SCR_WAVES;
constexpr int SCR_LDS_WORDS = 16384;                            // 64 KiB per workgroup: two workgroups per CU
constexpr int SCR_MAX_TILE = 64;
constexpr int SCR_CHUNK = 64;                                   // mask words per wave in the compaction
constexpr unsigned SCR_BAD_COUNT = 4u, SCR_NOT_ASCENDING = 8u;  // next to TAB_BAD_ID | TAB_DUPLICATE in TableStatus::flags

// words of LDS per staged signature: the power of two that holds s words (screen_pair, PADDED)
__host__ __device__ inline int screen_stride(int s) {
  int p = 1;
  while (p < s) p <<= 1;
  return p;
}

// genomes per tile side (its thresholds are powers of two themselves: a row's padding never costs a tile its size)
inline int screen_tile(int s) {
  int t = SCR_MAX_TILE;
  while (t > 2 && 2 * t * screen_stride(s) > SCR_LDS_WORDS) t >>= 1;
  return t;
}

// ---- signatures ------------------------------------------------------------------------------------------------------
struct SigArgs {
  const uint32_t *hash;
  const int32_t *seq_id;
  int64_t n_records;
  const int32_t *sbf;                  // device copy
  int32_t n_genomes, s;
  int32_t n_contigs;                   // sbf[n_genomes - 1]
  int32_t genome_bits;                 // k_sig_keys<true>: the bits of the largest genome number, below the hash
  const unsigned long long *keys;      // sorted
  const uint32_t *rank;                // exclusive scan of the heads
  uint32_t *first, *last;              // [n_genomes], zeroed: head ranks [first, last) of every genome with records
  uint32_t *sig;
  int32_t *count;
  TableStatus *status;
};

__global__ __launch_bounds__(256) void k_sig_check(SigArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_records) return;
  const int32_t c = a.seq_id[i];
  unsigned flags = 0;
  if ((uint32_t)c >= (uint32_t)a.n_contigs) flags |= TAB_BAD_ID;
  if (i > 0 && a.seq_id[i - 1] > c) flags |= SCR_NOT_ASCENDING;
  if (flags) atomicOr(&a.status->flags, flags);
}

// HASH_MAJOR: hash << genome_bits | genome, the order of a collection's contents (fa_contain.hip.h); else genome << 32 | hash
template <bool HASH_MAJOR>
__global__ __launch_bounds__(256) void k_sig_keys(SigArgs a, unsigned long long *keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_records) return;
  const int32_t c = a.seq_id[i];
  int lo = 0, hi = a.n_genomes;                                      // the first genome g with sbf[g] > c (k_sig_check: there is one)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.sbf[mid] > c) hi = mid; else lo = mid + 1;
  }
  const unsigned long long g = (unsigned long long)(uint32_t)min(lo, a.n_genomes - 1), h = a.hash[i];
  keys[i] = HASH_MAJOR ? h << a.genome_bits | g : g << 32 | h;
}

__global__ __launch_bounds__(256) void k_sig_heads(SigArgs a, uint32_t *heads) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.n_records) heads[i] = (i == 0 || a.keys[i] != a.keys[i - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_sig_segments(SigArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_records) return;
  const unsigned long long key = a.keys[i];
  const uint32_t g = (uint32_t)(key >> 32);
  const bool head = i == 0 || a.keys[i - 1] != key;
  if (i == 0 || (uint32_t)(a.keys[i - 1] >> 32) != g) a.first[g] = a.rank[i];
  if (i + 1 == a.n_records || (uint32_t)(a.keys[i + 1] >> 32) != g) a.last[g] = a.rank[i] + (head ? 1u : 0u);
}

__global__ __launch_bounds__(256) void k_sig_write(SigArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_records) return;
  const unsigned long long key = a.keys[i];
  if (i > 0 && a.keys[i - 1] == key) return;
  const uint32_t g = (uint32_t)(key >> 32);
  const uint32_t r = a.rank[i] - a.first[g];
  if (r < (uint32_t)a.s) a.sig[(size_t)g * (size_t)a.s + r] = (uint32_t)key;
}

__global__ __launch_bounds__(256) void k_sig_counts(SigArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g < a.n_genomes) a.count[g] = (int32_t)min(a.last[g] - a.first[g], (uint32_t)a.s);
}

// ---- pairs -----------------------------------------------------------------------------------------------------------
struct ScreenArgs {
  const uint32_t *sig_a, *sig_b;
  const int32_t *count_a, *count_b;
  int32_t n_a, n_b, s;
  int32_t tile, tile_shift, tiles_a;
  int32_t triangular;
  int32_t jn, jd;
  unsigned long long *mask;            // [n_a][words_per_row], zeroed: bit b of row a = the pair is kept
  int64_t words_per_row, n_words;
  int32_t n_chunks;
  int32_t *chunk_count;                // [n_chunks]
  int64_t *chunk_off;                  // [n_chunks]
  fa_screen_pair *pairs;
  TableStatus *status;
};

struct ScreenStat { int32_t shared, denom; };

// One wave, one pair: A and B are ascending distinct signatures of ca and cb words (LDS, B then PADDED, or global memory); every lane
// returns the same two counts.  All 64 lanes must be active.  A pass takes 64 * E elements of A, lane l the elements
// l, l + 64, ... of it: the E searches of a lane are independent chains of LDS reads, which is what hides their latency.
// PADDED: B is a row of LDS of screen_stride(s) words -- a power of two -- filled with 0xFFFFFFFF from cb on.  No hash is
// above that value, so a probe beyond cb never moves the lower bound and the search needs no test against cb: a step is
// an address, a read, a compare and a select.  The steps find a bound in [0, stride - 1]; the read of B at the bound, which
// the membership test needs anyway, tells the one case they cannot (a full row whose every element is below x).
template <int E, bool PADDED>
__device__ __forceinline__ ScreenStat screen_pair(const uint32_t *A, int ca, const uint32_t *B, int cb, int s, int lane) {
  const unsigned long long below = (1ULL << lane) - 1ULL;
  const int top = PADDED ? screen_stride(s) >> 1 : cb > 0 ? 1 << (31 - __clz(cb)) : 0;       // the first step of the search
  int matches = 0, shared = 0;
  bool full = false;
  for (int base = 0; base < ca && !full; base += 64 * E) {
    const int live = min(E, (ca - base + 63) >> 6);                // blocks of 64 that hold an element (uniform in the wave)
    uint32_t x[E];
    int lo[E];                                                     // the number of elements of B below x
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int i = base + 64 * e + lane;
      x[e] = i < ca ? A[i] : 0u;
      lo[e] = 0;
    }
    for (int half = top; half; half >>= 1) {                       // (not PADDED: top != 0 means B is not empty)
      uint32_t probe[E];
#pragma unroll
      for (int e = 0; e < E; e++) probe[e] = B[(PADDED ? lo[e] + half : min(lo[e] + half, cb)) - 1];      // E reads in flight
#pragma unroll
      for (int e = 0; e < E; e++)
        if ((PADDED || lo[e] + half <= cb) && probe[e] < x[e]) lo[e] += half;
    }
#pragma unroll
    for (int e = 0; e < E; e++) {
      if (e >= live || full) continue;
      const int i = base + 64 * e + lane;
      const uint32_t at = (PADDED || lo[e] < cb) ? B[lo[e]] : 0xFFFFFFFFu;
      if (PADDED && at < x[e]) lo[e]++;
      const bool match = i < ca && lo[e] < cb && at == x[e];
      const unsigned long long m = __ballot(match);
      const int rank = i + lo[e] - (matches + __popcll(m & below));
      if (__builtin_amdgcn_readfirstlane(rank) >= s) { full = true; continue; }   // (ranks ascend: nothing below s is left)
      shared += __popcll(__ballot(match && rank < s));
      matches += __popcll(m);
    }
  }
  ScreenStat st;
  st.shared = shared;
  st.denom = full ? s : min(s, ca + cb - matches);
  return st;
}

__device__ __forceinline__ bool screen_keep(const ScreenArgs &a, ScreenStat st) {
  return st.denom > 0 && (long long)st.shared * a.jd >= (long long)a.jn * st.denom;
}

// the count of a genome clamped to what its row of LDS holds (0 beyond the set); `bad`: it lies outside [0, s]
__device__ __forceinline__ int screen_count(const int32_t *count, int g, int n, int s, bool &bad) {
  if (g >= n) return 0;
  const int c = count[g];
  bad |= c < 0 || c > s;
  return min(max(c, 0), s);
}

template <int E>
__global__ __launch_bounds__(SCR_THREADS) void k_screen_pairs(ScreenArgs a) {
  extern __shared__ uint32_t sh_sig[];                               // [2 * tile][stride]: the A rows, then the B rows (padded)
  const int stride = screen_stride(a.s);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int T = a.tile, tb = blockIdx.x;
  for (int ta = blockIdx.y; ta < a.tiles_a; ta += gridDim.y) {
    if (a.triangular && ta > tb) continue;                           // (uniform in the workgroup)
    __syncthreads();                                                 // the tile before this one is done with
    bool bad_count = false, unordered = false;
    // lane l keeps the counts of the tile's A row l and B row l (T <= 64): a pair reads its two by lane number
    const int count_a = lane < T ? screen_count(a.count_a, ta * T + lane, a.n_a, a.s, bad_count) : 0;
    const int count_b = lane < T ? screen_count(a.count_b, tb * T + lane, a.n_b, a.s, bad_count) : 0;
    for (int row = wave; row < 2 * T; row += SCR_WAVES) {
      const int g = row < T ? ta * T + row : tb * T + row - T;
      const int c = row < T ? __shfl(count_a, row) : __shfl(count_b, row - T);
      const uint32_t *src = (row < T ? a.sig_a : a.sig_b) + (size_t)g * (size_t)a.s;
      uint32_t *dst = sh_sig + row * stride;
      for (int col = lane; col < c; col += 64) {
        const uint32_t v = src[col];
        if (col > 0 && src[col - 1] >= v) unordered = true;
        dst[col] = v;
      }
      if (row >= T)
        for (int col = c + lane; col < stride; col += 64) dst[col] = 0xFFFFFFFFu;
    }
    if (bad_count && wave == 0) atomicOr(&a.status->flags, SCR_BAD_COUNT);
    if (unordered) atomicOr(&a.status->flags, SCR_NOT_ASCENDING);
    __syncthreads();
    for (int p = wave; p < T * T; p += SCR_WAVES) {
      const int ia = p >> a.tile_shift, ib = p & (T - 1);
      const int ga = ta * T + ia, gb = tb * T + ib;
      if (ga >= a.n_a || gb >= a.n_b || (a.triangular && ga >= gb)) continue;            // (uniform in the wave)
      const int ca = __shfl(count_a, ia), cb = __shfl(count_b, ib);
      const ScreenStat st = screen_pair<E, true>(sh_sig + ia * stride, ca, sh_sig + (T + ib) * stride, cb, a.s, lane);
      if (lane == 0 && screen_keep(a, st)) atomicOr(a.mask + (int64_t)ga * a.words_per_row + (gb >> 6), 1ULL << (gb & 63));
    }
  }
}

__global__ __launch_bounds__(256) void k_screen_count(ScreenArgs a) {
  const int lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= a.n_chunks) return;                                   // (wave-uniform)
  const int64_t w = (int64_t)chunk * SCR_CHUNK + lane;
  int n = w < a.n_words ? __popcll(a.mask[w]) : 0;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) n += __shfl_xor(n, d);
  if (lane == 0) a.chunk_count[chunk] = n;
}

__global__ __launch_bounds__(256) void k_screen_write(ScreenArgs a) {
  const int lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= a.n_chunks || a.chunk_count[chunk] == 0) return;      // (wave-uniform)
  const int64_t w0 = (int64_t)chunk * SCR_CHUNK;
  const unsigned long long mine = w0 + lane < a.n_words ? a.mask[w0 + lane] : 0ULL;
  int64_t off = a.chunk_off[chunk];
  for (int u = 0; u < SCR_CHUNK; u++) {
    unsigned long long word = __shfl(mine, u);
    if (!word) continue;
    const int64_t w = w0 + u;
    const int32_t ga = (int32_t)(w / a.words_per_row);
    const int32_t b0 = (int32_t)(w - (int64_t)ga * a.words_per_row) * 64;
    while (word) {
      const int32_t gb = b0 + __ffsll((long long)word) - 1;
      word &= word - 1ULL;
      const ScreenStat st = screen_pair<1, false>(a.sig_a + (size_t)ga * (size_t)a.s, a.count_a[ga], a.sig_b + (size_t)gb * (size_t)a.s, a.count_b[gb],
                                        a.s, lane);
      if (lane == 0) {
        fa_screen_pair r;
        r.a = ga; r.b = gb; r.shared = st.shared; r.denom = st.denom;
        a.pairs[off] = r;
      }
      off++;
    }
  }
}

// ---- groups ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_screen_edges(const fa_screen_pair *pairs, int64_t n_pairs, int32_t n_genomes, int2 *edges,
                                                      TableStatus *status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pairs) return;
  const int32_t ea = pairs[i].a, eb = pairs[i].b;
  const bool good = ea >= 0 && ea < eb && eb < n_genomes;
  if (!good) atomicOr(&status->flags, TAB_BAD_ID);
  edges[i] = good ? make_int2(ea, eb) : make_int2(0, 0);
}

}  // namespace fa
