// fa_contain.hip.h -- the containment road of the screen: a collection's full distinct (hash, genome) sets laid out as one
// sorted directory (fa_screen_contents), and query signatures looked up in it, every (query, reference) reduced to the number
// of the query's elements the reference holds (fa_screen_contained).  Where the Jaccard road of fa_screen.hip.h collapses --
// a contig, a plasmid or an incomplete genome against the complete relative it is a part of -- this statistic does not: it
// is what `mash screen` computes.  Nothing here is on the mapping path: the kernels run only under those two entry points, on
// a stream of the call's own.
//
// Semantics
//   1. Contents of a collection.  Genome g owns the records whose contig id lies in [sbf[g-1], sbf[g]), exactly as for
//      signatures (fa_screen.hip.h).  The contents are the DISTINCT pairs (hash, genome) of the records, sorted ascending
//      by hash as unsigned 32-bit, then by genome.  Layout: uint32 ent_hash[m], int32 ent_genome[m]; m <= n_records; a
//      genome without records has no entry; 0 and 0xFFFFFFFF are legal hashes.
//   2. Statistic.  For a signature A (ascending, distinct, count_a long) and a reference genome b: shared = the number of
//      elements x of A with an entry (x, b); denom = count_a.  denom == 0 never forms a pair.
//   3. Filter.  A pair is kept iff denom > 0 and (int64)shared * cd >= (int64)cn * denom, cn / cd being the caller's
//      rational containment cut-off, 0 <= cn <= cd, cd >= 1, both int32: integers only, as in fa_screen_pairs.
//   4. Output.  fa_screen_pair { int32 a, b, shared, denom } sorted by (a, b), a indexing the signature set and b the
//      collection; every pair is rectangular.  The same input gives the same bytes on every run.
//
// Contents.  The road of the signatures with the key turned round: k_sig_check, then k_sig_keys<true> packs
// hash << id_bits | genome (id_bits: the bits of the largest genome number, so that the key has no idle bits between its
// two parts), one radix sort over 32 + id_bits bits, k_sig_heads marks the keys that differ from their predecessor, and the
// heads are compacted in order by count / scan / write over chunks of ENT_CHUNK keys (k_ent_count, the shared
// k_chunk_scan, k_ent_write: a head's place is its chunk's offset plus the population count of the ballots below its lane).
//
// Counting, the hot path.  Searching every reference's set for every pair costs s log|H_b| reads per pair; the directory
// turns that round, so that the work follows the matches and not the pairs.  A workgroup of CNT_WAVES waves owns one query a
// and one slice of CNT_SLICE references [g_lo, g_hi); its counters live in LDS, 16 bits per reference, two to a word
// (shared <= count_a <= 4096, and the entries (x, b) are distinct, so a half never carries into its neighbour).  A thread
// takes the elements tid, tid + T, ... of A, E at a time: E independent branch-free binary searches (64-bit indices, their
// reads issued together) find the lower bound of (x, g_lo) in the directory -- for the first slice that is the lower bound of x
// in ent_hash alone and the genomes are not read.  From there the run of entries (x, g), g < g_hi, is walked and every entry
// adds one to the counter of g: by the lane itself for the first CNT_LANE_RUN entries, and, where a run goes on beyond that -- a
// hash that sits in thousands of strains is the normal case -- by the whole wave, lane per entry, one unfinished run after the
// other.  Every entry walked is one of the slice, so the entries visited are the same number however the references are sliced.
// After a barrier wave w passes over the counters of its eighth of the slice in b order, 64 references at a time, and applies
// the filter.  The COUNT form stores the number kept per (a, slice); k_chunk_scan over those numbers, a-major, gives every
// workgroup its base; the WRITE form recomputes the counters and stores the kept records at base + the kept of the waves
// before + the population count of the ballots below the lane.  No atomic decides a record's place (the LDS adds only sum).
// k_contain_check runs before either: counts in [0, s], signatures strictly ascending, entries strictly ascending by (hash,
// genome) with genomes in [0, n_b), weights not negative -- the host reads its flags before a counting kernel is launched, so
// those may rely on them.
//
// Winner take all (fa_screen_contained_winner).  A query of a well-sampled species is held by every strain; here every element
// of A is credited to ONE reference and the records carry what a reference won.  It is the library's integer restatement of
// `mash screen -w`, over the winnowed minimizers, and has not been checked against the Mash program.
//   1. First pass.  first[b] = the number of x in A with an entry (x, b): the plain `shared`, over all references.
//   2. Winner.  For x in A with at least one entry, winner(x) = the b with the largest first[b] among those with an entry
//      (x, b), whether they pass the cut-off or not; ties go to the largest weight[b] (int32 >= 0 per reference, all 0 without
//      a weight array), remaining ties to the smallest b.  denom is the same for every b: integers compare the identities.
//   3. Statistic.  won[b] = the number of x in A with winner(x) == b; denom = count_a.
//   4. Filter and output.  As above with won in the place of shared (cn == 0 keeps won == 0); the same bytes on every run.
// The credits need the first-pass counts of ALL references of a query, so they are a second, dependent walk of the directory.
// k_contain_winner takes one workgroup per query and the slices one after the other: per slice the counting walk above into
// the same 16-bit counters, a barrier, and the same runs walked again, every run reduced to its best (first, weight, smallest
// g) and merged into the element's running best, which lives in LDS next to the counters together with the place where the
// element's entries of the next slice begin -- the directory is searched once per element, not once per slice.  No atomic
// decides a winner: a lane-walked run reduces in registers, a wave-walked one by butterflies in a fixed order, and an element
// belongs to one thread.  It stores winner[a][i] (-1: no entry) once per call; k_contain_won, on the grid of k_contain and with
// its epilogue (contain_emit), counts the winners that lie in its slice for the COUNT and for the WRITE form.  LDS: the counters
// (<= 65 408 B) and 20 bytes per element of the signature (<= 80 KiB), beyond 64 KiB for a large collection or signature: the
// launch raises hipFuncAttributeMaxDynamicSharedMemorySize, and a CU holds one such workgroup out of its 160 KiB.  512 or 1024
// threads per workgroup: 512 (WIN_THREADS).  scripts/time_contain_winner.py times both, and 1024 was 4-6 % slower on its two
// collections (profiles/contain_winner_timing.json: 1.20 against 1.25 ms for 1 000 queries at s = 1000 over 10 000 references).
#pragma once

#include <type_traits>

#include "fa_screen.hip.h"

namespace fa {

constexpr int CNT_WAVES = 8, CNT_THREADS = 64 * CNT_WAVES;
// references per workgroup: with the eight words of sh_wave just within 64 KiB of LDS, so that two workgroups fit a CU
constexpr int CNT_SLICE = 32768 - 64;
constexpr int CNT_LANE_RUN = 64;                                // entries of a run a lane walks by itself
constexpr int ENT_ITERS = 8, ENT_CHUNK = 64 * ENT_ITERS;        // keys per wave in the compaction of the contents
constexpr unsigned CNT_UNORDERED = 16u, CNT_BAD_WEIGHT = 32u;   // next to TAB_BAD_ID | SCR_BAD_COUNT | SCR_NOT_ASCENDING
constexpr int WIN_THREADS = 512;                                // of k_contain_winner; 1024, its other form, measured slower (above)

// one per call, zeroed before the first launch
struct ContainStatus {
  int64_t emitted;                     // k_chunk_scan: records the WRITE form produces
  unsigned long long visited;          // directory entries walked by the COUNT form (k_contain_winner: by its counting walks)
  unsigned int flags, pad;
  unsigned long long assigned;         // k_contain_winner: elements that have a winner
};

// ---- contents --------------------------------------------------------------------------------------------------------
struct EntArgs {
  const unsigned long long *keys;      // sorted: hash << genome_bits | genome
  const uint32_t *heads;               // k_sig_heads
  int64_t n_records;
  int32_t n_chunks, genome_bits;
  int32_t *chunk_count;                // [n_chunks]
  int64_t *chunk_off;                  // [n_chunks]
  uint32_t *ent_hash;
  int32_t *ent_genome;
};

__global__ __launch_bounds__(256) void k_ent_count(EntArgs a) {
  const int lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= a.n_chunks) return;                                   // (wave-uniform)
  const int64_t i0 = (int64_t)chunk * ENT_CHUNK + lane;
  int n = 0;
#pragma unroll
  for (int it = 0; it < ENT_ITERS; it++) {
    const int64_t i = i0 + 64 * it;
    n += i < a.n_records ? (int)a.heads[i] : 0;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) n += __shfl_xor(n, d);
  if (lane == 0) a.chunk_count[chunk] = n;
}

__global__ __launch_bounds__(256) void k_ent_write(EntArgs a) {
  const int lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= a.n_chunks || a.chunk_count[chunk] == 0) return;      // (wave-uniform)
  const unsigned long long below = (1ULL << lane) - 1ULL;
  const int64_t i0 = (int64_t)chunk * ENT_CHUNK + lane;
  int64_t off = a.chunk_off[chunk];
  for (int it = 0; it < ENT_ITERS; it++) {
    const int64_t i = i0 + 64 * it;
    const bool head = i < a.n_records && a.heads[i] != 0u;
    const unsigned long long m = __ballot(head);
    if (head) {
      const unsigned long long key = a.keys[i];
      const int64_t at = off + __popcll(m & below);
      a.ent_hash[at] = (uint32_t)(key >> a.genome_bits);
      a.ent_genome[at] = (int32_t)(key & ((1ULL << a.genome_bits) - 1ULL));
    }
    off += __popcll(m);
  }
}

// ---- containment -----------------------------------------------------------------------------------------------------
struct ContainArgs {
  const uint32_t *sig;
  const int32_t *count;
  int32_t n_a, s;
  const uint32_t *ent_hash;
  const int32_t *ent_genome;
  int64_t m;
  int32_t n_b, n_slices;
  int32_t cn, cd;
  const int32_t *weight;               // [n_b] or null (every weight 0): the winner rule's second key
  int32_t *winner;                     // [n_a * s]: k_contain_winner's verdict per element, -1 without an entry
  int32_t *group_count;                // [n_a * n_slices], a-major: the records of every (a, slice)
  int64_t *group_off;                  // their exclusive scan
  fa_screen_pair *pairs;
  ContainStatus *status;
};

__global__ __launch_bounds__(256) void k_contain_check(ContainArgs a) {
  const int64_t n_sig = (int64_t)a.n_a * a.s, n_weights = a.weight ? a.n_b : 0;
  const int64_t total = max(max(n_sig, a.m), n_weights);
  unsigned flags = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    if (i < n_sig) {
      const int64_t g = i / a.s;
      const int32_t col = (int32_t)(i - g * a.s), c = a.count[g];
      if (col == 0 && (c < 0 || c > a.s)) flags |= SCR_BAD_COUNT;
      if (col > 0 && col < min(c, a.s) && a.sig[i - 1] >= a.sig[i]) flags |= SCR_NOT_ASCENDING;
    }
    if (i < a.m) {
      const uint32_t h = a.ent_hash[i];
      const int32_t g = a.ent_genome[i];
      if ((uint32_t)g >= (uint32_t)a.n_b) flags |= TAB_BAD_ID;
      if (i > 0) {
        const uint32_t hp = a.ent_hash[i - 1];
        if (hp > h || (hp == h && a.ent_genome[i - 1] >= g)) flags |= CNT_UNORDERED;
      }
    }
    if (i < n_weights && a.weight[i] < 0) flags |= CNT_BAD_WEIGHT;
  }
  if (flags) atomicOr(&a.status->flags, flags);
}

__device__ __forceinline__ bool contain_keep(const ContainArgs &a, int shared, int denom) {
  return (long long)shared * a.cd >= (long long)a.cn * denom;         // (denom > 0: a query without elements has left before)
}

// The workgroup of k_contain and k_contain_won: one query and one slice of the references, CNT_THREADS threads.
struct ContainGroup {
  int ga, ca;                          // the query and its count
  int32_t g_lo, g_hi;                  // the slice
  int width;
};

// false: the workgroup has nothing to do (uniform in the workgroup); else the counters are zeroed and a barrier has passed
template <bool WRITE>
__device__ __forceinline__ bool contain_group(const ContainArgs &a, uint32_t *sh_cnt, ContainGroup &w) {
  const int tid = threadIdx.x;
  w.ga = (int)(blockIdx.x / (unsigned)a.n_slices);
  const int slice = (int)(blockIdx.x - (unsigned)w.ga * (unsigned)a.n_slices);
  w.g_lo = slice * CNT_SLICE;
  w.g_hi = (int32_t)min((long long)a.n_b, (long long)w.g_lo + CNT_SLICE);
  w.width = w.g_hi - w.g_lo;
  w.ca = a.count[w.ga];
  if (WRITE && a.group_count[blockIdx.x] == 0) return false;
  if (w.ca == 0) {
    if (!WRITE && tid == 0) a.group_count[blockIdx.x] = 0;
    return false;
  }
  for (int i = tid; i < (w.width + 1) >> 1; i += CNT_THREADS) sh_cnt[i] = 0u;
  __syncthreads();
  return true;
}

// The epilogue of both, once the LDS adds are issued: after a barrier wave w passes over the counters of its eighth of the
// slice in b order and applies the filter; the COUNT form stores the number kept, the WRITE form the records at their base.
template <bool WRITE>
__device__ __forceinline__ void contain_emit(const ContainArgs &a, const uint32_t *sh_cnt, int *sh_wave, const ContainGroup &w) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int width = w.width, ca = w.ca;
  __syncthreads();
  // wave w owns the references [r0, r1) of the slice, 64 at a time in b order
  const unsigned long long below = (1ULL << lane) - 1ULL;
  const int seg = (width + CNT_THREADS - 1) / CNT_THREADS * 64;
  const int r0 = min(width, wave * seg), r1 = min(width, r0 + seg);
  auto shared_of = [&](int r) { return (int)((sh_cnt[r >> 1] >> ((r & 1) * 16)) & 0xFFFFu); };
  int kept = 0;
  for (int rb = r0; rb < r1; rb += 64) {
    const int r = rb + lane;
    kept += __popcll(__ballot(r < r1 && contain_keep(a, shared_of(r), ca)));
  }
  if (lane == 0) sh_wave[wave] = kept;
  __syncthreads();
  if (!WRITE) {
    if (tid == 0) {
      int total = 0;
      for (int v = 0; v < CNT_WAVES; v++) total += sh_wave[v];
      a.group_count[blockIdx.x] = total;
    }
  } else {
    int64_t off = a.group_off[blockIdx.x];
    for (int v = 0; v < wave; v++) off += sh_wave[v];
    for (int rb = r0; rb < r1; rb += 64) {
      const int r = rb + lane;
      const int shared = r < r1 ? shared_of(r) : 0;
      const bool keep = r < r1 && contain_keep(a, shared, ca);
      const unsigned long long k = __ballot(keep);
      if (keep) {
        fa_screen_pair rec;
        rec.a = w.ga; rec.b = w.g_lo + r; rec.shared = shared; rec.denom = ca;
        a.pairs[off + __popcll(k & below)] = rec;
      }
      off += __popcll(k);
    }
  }
}

template <int E, bool WRITE>
__global__ __launch_bounds__(CNT_THREADS) void k_contain(ContainArgs a) {
  extern __shared__ uint32_t sh_cnt[];                               // [(width + 1) / 2]: reference g_lo + r in half r & 1 of word r >> 1
  __shared__ int sh_wave[CNT_WAVES];
  const int tid = threadIdx.x, lane = tid & 63;
  ContainGroup w;
  if (!contain_group<WRITE>(a, sh_cnt, w)) return;                   // (uniform in the workgroup)
  const int ga = w.ga, ca = w.ca, width = w.width;
  const int32_t g_lo = w.g_lo, g_hi = w.g_hi;

  const uint32_t *A = a.sig + (size_t)ga * (size_t)a.s;
  const int64_t m = a.m;
  const int64_t top = m > 0 ? (int64_t)1 << (63 - __clzll((long long)m)) : 0;      // the first step of the search
  int visited = 0;
  // one entry (x, g) of the slice found: g's counter goes up by one
  auto add = [&](int32_t g) {
    const unsigned r = (unsigned)(g - g_lo);
    if (r < (unsigned)width) atomicAdd(&sh_cnt[r >> 1], 1u << ((r & 1u) * 16u));
    visited++;
  };
  for (int base = 0; base < ca; base += CNT_THREADS * E) {            // (uniform in the workgroup)
    uint32_t x[E];
    int64_t lo[E];                                                    // the number of entries below (x, g_lo)
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int i = base + CNT_THREADS * e + tid;
      x[e] = i < ca ? A[i] : 0u;
      lo[e] = 0;
    }
    for (int64_t half = top; half; half >>= 1) {
      uint32_t ph[E];
      int32_t pg[E];
#pragma unroll
      for (int e = 0; e < E; e++) {                                   // E (or 2 E) reads in flight
        const int64_t at = (lo[e] + half <= m ? lo[e] + half : m) - 1;
        ph[e] = a.ent_hash[at];
        pg[e] = g_lo ? a.ent_genome[at] : 0;
      }
#pragma unroll
      for (int e = 0; e < E; e++)
        if (lo[e] + half <= m && (ph[e] < x[e] || (ph[e] == x[e] && pg[e] < g_lo))) lo[e] += half;
    }
#pragma unroll
    for (int e = 0; e < E; e++) {
      const bool live = base + CNT_THREADS * e + tid < ca;
      int64_t at = lo[e];
      int32_t g = 0;
      auto inside = [&]() {                                           // `at` is an entry (x, g) of the slice
        if (!(at < m && a.ent_hash[at] == x[e])) return false;
        g = a.ent_genome[at];
        return g < g_hi;
      };
      bool more = live && inside();
      for (int j = 0; more && j < CNT_LANE_RUN; j++) {
        add(g);
        at++;
        more = inside();
      }
      // the runs that go on: the wave walks them one after the other, lane per entry
      unsigned long long longer = __ballot(more);
      while (longer) {                                                // (wave-uniform)
        const int src = __ffsll((long long)longer) - 1;
        longer &= longer - 1ULL;
        const int64_t start = __shfl(at, src);
        const uint32_t xs = __shfl(x[e], src);
        for (int64_t p = start;; p += 64) {
          const int64_t q = p + lane;
          bool in = q < m && a.ent_hash[q] == xs;
          const int32_t gq = in ? a.ent_genome[q] : 0;
          in = in && gq < g_hi;
          if (in) add(gq);
          if (!__all(in)) break;
        }
      }
    }
  }
  contain_emit<WRITE>(a, sh_cnt, sh_wave, w);
  if (!WRITE) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) visited += __shfl_xor(visited, d);
    if (lane == 0 && visited) atomicAdd(&a.status->visited, (unsigned long long)visited);
  }
}

// ---- winner take all -------------------------------------------------------------------------------------------------
// One workgroup of T threads per query, the slices of the references one after the other.  Element i of A belongs to thread
// i % T from start to end, so its words of LDS need no barrier: only the counters do.
//   sh_at[i]   where the entries (A[i], g >= g_lo) begin: the lower bound of A[i] in ent_hash, searched ONCE (E chains per
//              thread), then the end of the run of every slice walked -- the entries of a hash ascend in g
//   sh_key[i]  first << 32 | weight of the running winner, 0: none yet;  sh_g[i] its number, -1: none yet
//   sh_cnt     the 16-bit counters of the slice, as in k_contain
// Per slice: the counting walk of k_contain (`first` of the slice), a barrier, then the same runs walked again, every run
// reduced to its largest key and the smallest g that has it -- in the lane's registers for the first CNT_LANE_RUN entries, and
// for a run that goes on by the wave, lane per entry: every lane keeps its own best (its g ascend from trip to trip), then the
// maximum of the keys and the minimum g among the lanes that hold it are taken by xor butterflies, a fixed order.  Slices ascend
// in g, so only a strictly larger key replaces the running winner.
template <int T, int E>
__global__ __launch_bounds__(T) void k_contain_winner(ContainArgs a) {
  extern __shared__ unsigned long long sh_win[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int ga = blockIdx.x, ca = a.count[ga];
  if (ca == 0) return;                                               // (uniform in the workgroup)
  int64_t *sh_at = reinterpret_cast<int64_t *>(sh_win);
  unsigned long long *sh_key = sh_win + a.s;
  int32_t *sh_g = reinterpret_cast<int32_t *>(sh_win + 2 * (size_t)a.s);
  uint32_t *sh_cnt = reinterpret_cast<uint32_t *>(sh_g + a.s);

  const uint32_t *A = a.sig + (size_t)ga * (size_t)a.s;
  const int64_t m = a.m;
  const int64_t top = m > 0 ? (int64_t)1 << (63 - __clzll((long long)m)) : 0;
  for (int base = 0; base < ca; base += T * E) {                      // (uniform in the workgroup)
    uint32_t x[E];
    int64_t lo[E];                                                    // the number of entries below x
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int i = base + T * e + tid;
      x[e] = i < ca ? A[i] : 0u;
      lo[e] = 0;
    }
    for (int64_t half = top; half; half >>= 1) {
      uint32_t ph[E];
#pragma unroll
      for (int e = 0; e < E; e++) ph[e] = a.ent_hash[(lo[e] + half <= m ? lo[e] + half : m) - 1];       // E reads in flight
#pragma unroll
      for (int e = 0; e < E; e++)
        if (lo[e] + half <= m && ph[e] < x[e]) lo[e] += half;
    }
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int i = base + T * e + tid;
      if (i < ca) { sh_at[i] = lo[e]; sh_key[i] = 0ULL; sh_g[i] = -1; }
    }
  }

  unsigned long long visited = 0;
  for (long long lo = 0; lo < a.n_b; lo += CNT_SLICE) {               // (uniform in the workgroup)
    const int32_t g_lo = (int32_t)lo, g_hi = (int32_t)min((long long)a.n_b, lo + CNT_SLICE);
    const int width = g_hi - g_lo;
    for (int i = tid; i < (width + 1) >> 1; i += T) sh_cnt[i] = 0u;
    __syncthreads();
    // best == false: every entry of the slice adds one to its reference; true: every run is reduced to its winner
    auto walk = [&](auto best_tag) {
      constexpr bool BEST = decltype(best_tag)::value;
      auto entry = [&](int32_t g, unsigned long long &key, int32_t &bg) {
        const unsigned r = (unsigned)(g - g_lo);
        if (r >= (unsigned)width) return;                             // (never: the walk starts where the slice before ended)
        if constexpr (!BEST) {
          atomicAdd(&sh_cnt[r >> 1], 1u << ((r & 1u) * 16u));
          visited++;
        } else {
          const unsigned long long first = (sh_cnt[r >> 1] >> ((r & 1u) * 16u)) & 0xFFFFu;
          const unsigned long long k = first << 32 | (a.weight ? (uint32_t)a.weight[g] : 0u);
          if (k > key) { key = k; bg = g; }
        }
      };
      for (int base = 0; base < ca; base += T) {                      // (uniform in the workgroup)
        const int i = base + tid;
        const bool live = i < ca;
        const uint32_t x = live ? A[i] : 0u;
        int64_t at = live ? sh_at[i] : m;
        int32_t g = 0, bg = -1;
        unsigned long long key = 0ULL;
        auto inside = [&]() {                                         // `at` is an entry (x, g) of the slice
          if (!(at < m && a.ent_hash[at] == x)) return false;
          g = a.ent_genome[at];
          return g < g_hi;
        };
        bool more = live && inside();
        for (int j = 0; more && j < CNT_LANE_RUN; j++) {
          entry(g, key, bg);
          at++;
          more = inside();
        }
        unsigned long long longer = __ballot(more);
        while (longer) {                                              // (wave-uniform)
          const int src = __ffsll((long long)longer) - 1;
          longer &= longer - 1ULL;
          const int64_t start = __shfl(at, src);
          const uint32_t xs = __shfl(x, src);
          unsigned long long wkey = 0ULL;
          int32_t wg = 0x7FFFFFFF;
          int64_t end = start;
          for (int64_t p = start;; p += 64) {
            const int64_t q = p + lane;
            bool in = q < m && a.ent_hash[q] == xs;
            const int32_t gq = in ? a.ent_genome[q] : 0;
            in = in && gq < g_hi;
            if (in) entry(gq, wkey, wg);
            const unsigned long long ins = __ballot(in);              // (a prefix of the lanes: the run is contiguous)
            if (ins != ~0ULL) { end = p + __popcll(ins); break; }
          }
          if constexpr (BEST) {
            unsigned long long mkey = wkey;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const unsigned long long o = __shfl_xor(mkey, d); mkey = o > mkey ? o : mkey; }
            int32_t mg = wkey == mkey ? wg : 0x7FFFFFFF;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) mg = min(mg, __shfl_xor(mg, d));
            if (lane == src) {
              if (mkey > key) { key = mkey; bg = mg; }                // (the lane's own entries come first: smaller g)
              at = end;
            }
          }
        }
        if constexpr (BEST) if (live) {
          sh_at[i] = at;                                              // where the next slice's entries of x begin
          if (key > sh_key[i]) { sh_key[i] = key; sh_g[i] = bg; }
        }
      }
    };
    walk(std::false_type{});
    __syncthreads();
    walk(std::true_type{});
    __syncthreads();                                                  // (the counters are zeroed again)
  }

  int32_t *W = a.winner + (size_t)ga * (size_t)a.s;
  unsigned long long assigned = 0;
  for (int i = tid; i < ca; i += T) {
    const int32_t g = sh_g[i];
    W[i] = g;
    assigned += g >= 0;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { visited += __shfl_xor(visited, d); assigned += __shfl_xor(assigned, d); }
  if (lane == 0 && visited) atomicAdd(&a.status->visited, visited);
  if (lane == 0 && assigned) atomicAdd(&a.status->assigned, assigned);
}

// One workgroup per (query, slice), the grid and the epilogue of k_contain: the counters receive one per element of the query
// whose winner lies in the slice.
template <bool WRITE>
__global__ __launch_bounds__(CNT_THREADS) void k_contain_won(ContainArgs a) {
  extern __shared__ uint32_t sh_cnt[];
  __shared__ int sh_wave[CNT_WAVES];
  ContainGroup w;
  if (!contain_group<WRITE>(a, sh_cnt, w)) return;                   // (uniform in the workgroup)
  const int32_t *W = a.winner + (size_t)w.ga * (size_t)a.s;
  for (int i = threadIdx.x; i < w.ca; i += CNT_THREADS) {
    const unsigned r = (unsigned)W[i] - (unsigned)w.g_lo;             // (-1, no winner, lies in no slice)
    if (r < (unsigned)w.width) atomicAdd(&sh_cnt[r >> 1], 1u << ((r & 1u) * 16u));
  }
  contain_emit<WRITE>(a, sh_cnt, sh_wave, w);
}

}  // namespace fa
