// fa_select.hip.h -- a subset of a sketch's genomes cut out on the device into a sketch of its own (fa_sketch_select), and
// the pieces of fa_sketch_frequency that are not rocPRIM calls.  A collection larger than one index is mapped group by group
// out of ONE resident sketch this way: the groups come from the screen (fa_screen.hip.h), every group's records from here, and
// the frequency filter of the whole collection -- which makes a group's rows those of the one big index, DESIGN.md -- from
// fa_sketch_frequency.  Nothing here is on the mapping path: the kernels run only under those two entry points, on the
// sketch's stream.
//
// Semantics (select)
//   With sbf = sequencesByFileInfo of the source, first(g) = g ? sbf[g-1] : 0 and c(g) = sbf[g] - first(g), the selection
//   genomes[0..n) (strictly ascending, every entry in [0, n_genomes)) gives a sketch with
//     lengths'[i] = lengths[genomes[i]],  sbf'[i] = sum over j <= i of c(genomes[j]),  counter' = sbf'[n-1] (0 for n == 0).
//   Genome g owns the records whose contig id lies in [first(g), sbf[g]): a contiguous range, because records are sorted by
//   contig id.  The records of genomes[i] are copied in their order, hash and wpos unchanged, contig id
//   seq_id - first(genomes[i]) + first'(i).  The source is only read.
//
// The road.  The host turns the selection into one contig range and one contig-id shift per selected genome (segment).
// k_select_bounds finds the record range of every segment by two binary searches over the source's contig ids; the host
// scans the n segment lengths (a genome list is small next to the records, and a 64-bit device scan would be the one kernel
// of the library that needs scratch memory) and sizes the destination.  k_select_copy then runs over the OUTPUT records,
// so the cost goes with what is selected, not with the sketch: a workgroup takes SEL_TILE consecutive output records per
// trip, two of its threads find the segments of the tile's first and last record in the scanned offsets, and every record
// finds its own segment between those two -- no step at all where a tile lies inside one genome, which is the rule.  Lane l
// of a wave reads and writes record base + l of each of the three arrays: every access of a wave is 256 contiguous bytes on
// both sides (source and destination ranges are not aligned to each other, so wider accesses per lane would straddle
// segments).  The SEL_PER_THREAD records of a thread are read before any is written.  Record indices are 64-bit throughout:
// a sketch may hold more records than an index can.
//
// Frequency.  fa_sketch_frequency sorts a copy of the hashes, run-length encodes them, takes the threshold with the walk
// that build_index uses (frequency_threshold, fa_index.hip.h) and compacts the keys whose run reaches it: all rocPRIM, but
// for the predicate below.
#pragma once

#include <rocprim/rocprim.hpp>

#include <climits>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include "fa_common.h"
#include "fa_index.hip.h"
#include "fa_refsketch.hip.h"

namespace fa {

constexpr int SEL_THREADS = 256, SEL_PER_THREAD = 4;
constexpr int SEL_TILE = SEL_THREADS * SEL_PER_THREAD;          // output records per workgroup trip
constexpr int SEL_MAX_BLOCKS = 2048;                            // the grid strides over the tiles beyond

// rec_lo[i] / rec_hi[i] = first record with contig id >= contig_lo[i] / contig_hi[i]
__global__ void k_select_bounds(const int32_t *__restrict__ rec_seq, int64_t N, const int32_t *__restrict__ contig_lo,
                                const int32_t *__restrict__ contig_hi, int32_t n, int64_t *__restrict__ rec_lo, int64_t *__restrict__ rec_hi) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * (int64_t)n) return;
  const bool upper = t >= n;
  const int32_t i = (int32_t)(upper ? t - n : t);
  const int32_t c = upper ? contig_hi[i] : contig_lo[i];
  int64_t lo = 0, hi = N;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (rec_seq[mid] < c) lo = mid + 1; else hi = mid; }
  (upper ? rec_hi : rec_lo)[i] = lo;
}

struct SelectArgs {
  const uint32_t *src_hash;
  const int32_t *src_seq, *src_wpos;
  uint32_t *dst_hash;
  int32_t *dst_seq, *dst_wpos;
  const int64_t *dst_off;        // [n + 1] first output record of every segment, dst_off[n] = total
  const int64_t *src_lo;         // [n] first source record of every segment
  const int32_t *delta;          // [n] what a segment adds to its contig ids
  int32_t n;
  int64_t total;
};

// the last segment i in [lo, hi) with off[i] <= o; off[lo] <= o < off[hi] on entry.  An empty segment shares its offset with
// its successor and is never the answer.
__device__ inline int32_t select_segment(const int64_t *__restrict__ off, int32_t lo, int32_t hi, int64_t o) {
  while (hi - lo > 1) { const int32_t mid = lo + ((hi - lo) >> 1); if (off[mid] <= o) lo = mid; else hi = mid; }
  return lo;
}

__global__ __launch_bounds__(SEL_THREADS) void k_select_copy(SelectArgs a) {
  __shared__ int32_t sh_seg[2];
  const int64_t ntiles = (a.total + SEL_TILE - 1) / SEL_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t o0 = tile * SEL_TILE, o1 = min(o0 + (int64_t)SEL_TILE, a.total);
    if (threadIdx.x < 2) sh_seg[threadIdx.x] = select_segment(a.dst_off, 0, a.n, threadIdx.x ? o1 - 1 : o0);
    __syncthreads();
    const int32_t seg_lo = sh_seg[0], seg_hi = sh_seg[1];
    __syncthreads();                                            // (the next trip writes sh_seg again)
    uint32_t h[SEL_PER_THREAD];
    int32_t q[SEL_PER_THREAD], w[SEL_PER_THREAD];
#pragma unroll
    for (int j = 0; j < SEL_PER_THREAD; j++) {
      const int64_t o = o0 + (int64_t)j * SEL_THREADS + threadIdx.x;
      if (o < o1) {
        const int32_t seg = select_segment(a.dst_off, seg_lo, seg_hi + 1, o);
        const int64_t src = a.src_lo[seg] + (o - a.dst_off[seg]);
        h[j] = a.src_hash[src];
        q[j] = a.src_seq[src] + a.delta[seg];
        w[j] = a.src_wpos[src];
      }
    }
#pragma unroll
    for (int j = 0; j < SEL_PER_THREAD; j++) {
      const int64_t o = o0 + (int64_t)j * SEL_THREADS + threadIdx.x;
      if (o < o1) { a.dst_hash[o] = h[j]; a.dst_seq[o] = q[j]; a.dst_wpos[o] = w[j]; }
    }
  }
}

// the flag of a distinct hash in the compaction of fa_sketch_frequency: its list reaches the threshold
struct ListAtLeast {
  uint32_t threshold;
  __host__ __device__ bool operator()(uint32_t count) const { return count >= threshold; }
};

}  // namespace fa

// ------------------------------------------------------------------------------------------------------------
// host drivers (the entry points fa_sketch_select and fa_sketch_frequency wrap them; s->mtx is taken here)
// ------------------------------------------------------------------------------------------------------------
using namespace fa;

static void sketch_select(fa_sketch *s, const int32_t *genomes, int32_t n, fa_sketch **out) {
  FA_REQUIRE(s && out && n >= 0 && (genomes || n == 0), FA_ERR_INVALID, "null sketch, list or destination, or a negative count");
  std::lock_guard<std::mutex> lock(s->mtx);
  bind_device(s->device);
  const RefBook &book = s->book;
  const int64_t G = (int64_t)book.lengths.size();
  FA_REQUIRE(book.counter == (G ? (int64_t)book.seqs_by_file.back() : 0), FA_ERR_INVALID, "a genome is still open (add_contig without end_genome)");
  for (int32_t i = 0; i < n; i++) {
    FA_REQUIRE(genomes[i] >= 0 && genomes[i] < G, FA_ERR_INVALID, "a selected genome is outside [0, n_genomes)");
    FA_REQUIRE(i == 0 || genomes[i] > genomes[i - 1], FA_ERR_INVALID, "the selected genomes must ascend strictly");
  }
  require_device();
  s->flush();
  bind_device(s->device);
  std::unique_ptr<fa_sketch> o(new fa_sketch());
  o->P = s->P;
  o->device = s->device;
  o->reset_data();
  // one segment per selected genome: its contig range in the source and what its contig ids move by
  std::vector<int32_t> contig_lo((size_t)n), contig_hi((size_t)n), delta((size_t)n);
  int32_t contigs = 0;
  for (int32_t i = 0; i < n; i++) {
    const int32_t g = genomes[i];
    contig_lo[(size_t)i] = g ? book.seqs_by_file[(size_t)g - 1] : 0;
    contig_hi[(size_t)i] = book.seqs_by_file[(size_t)g];
    delta[(size_t)i] = contigs - contig_lo[(size_t)i];
    contigs += contig_hi[(size_t)i] - contig_lo[(size_t)i];
    o->book.lengths.push_back(book.lengths[(size_t)g]);
    o->book.seqs_by_file.push_back(contigs);
  }
  o->book.counter = contigs;
  if (n > 0 && s->nrec > 0) {
    require_device();
    hipStream_t st = s->stream.get();
    DevBuf<int32_t> d_contig_lo, d_contig_hi, d_delta;
    DevBuf<int64_t> d_rec, d_off;                             // d_rec: [n] first records, then [n] ends
    d_contig_lo.upload(contig_lo, st); d_contig_hi.upload(contig_hi, st);
    d_rec.ensure(2 * (size_t)n);
    hipLaunchKernelGGL(k_select_bounds, dim3(ceil_div(2 * (int64_t)n, 256)), dim3(256), 0, st, s->rec.seq.p, s->nrec, d_contig_lo.p, d_contig_hi.p, n,
                       d_rec.p, d_rec.p + n);
    FA_HIP(hipGetLastError());
    std::vector<int64_t> rec(2 * (size_t)n), off((size_t)n + 1);
    d_rec.download(rec.data(), rec.size(), st);
    FA_HIP(hipStreamSynchronize(st));
    int64_t total = 0;
    for (int32_t i = 0; i < n; i++) {
      const int64_t lo = rec[(size_t)i], hi = rec[(size_t)n + (size_t)i];
      FA_REQUIRE(0 <= lo && lo <= hi && hi <= s->nrec, FA_ERR_INTERNAL, "the records of the sketch are not sorted by contig id");
      off[(size_t)i] = total;
      total += hi - lo;
    }
    off[(size_t)n] = total;
    if (total > 0) {
      o->rec.hash.ensure((size_t)total); o->rec.seq.ensure((size_t)total); o->rec.wpos.ensure((size_t)total);
      d_off.upload(off, st); d_delta.upload(delta, st);
      SelectArgs a;
      a.src_hash = s->rec.hash.p; a.src_seq = s->rec.seq.p; a.src_wpos = s->rec.wpos.p;
      a.dst_hash = o->rec.hash.p; a.dst_seq = o->rec.seq.p; a.dst_wpos = o->rec.wpos.p;
      a.dst_off = d_off.p; a.src_lo = d_rec.p; a.delta = d_delta.p; a.n = n; a.total = total;
      const int64_t tiles = (total + SEL_TILE - 1) / SEL_TILE;
      hipLaunchKernelGGL(k_select_copy, dim3((unsigned)std::min<int64_t>(tiles, SEL_MAX_BLOCKS)), dim3(SEL_THREADS), 0, st, a);
      FA_HIP(hipGetLastError());
      FA_HIP(hipStreamSynchronize(st));
    }
    o->nrec = total;
  }
  *out = o.release();
}

static void sketch_frequency(fa_sketch *s, int *threshold, int64_t cap, uint32_t *d_drop_keys, int64_t *n_drop) {
  FA_REQUIRE(s && threshold && n_drop && cap >= 0 && (d_drop_keys || cap == 0), FA_ERR_INVALID, "null sketch or destination, or a negative capacity");
  std::lock_guard<std::mutex> lock(s->mtx);
  bind_device(s->device);
  require_device();
  s->flush();
  bind_device(s->device);
  const int64_t N = s->nrec;
  // (the list lengths are uint32, as in the index; nothing here is a record NUMBER, so 2^31 is no bound)
  FA_REQUIRE(N <= (int64_t)UINT32_MAX, FA_ERR_UNSUPPORTED, "more than 2^32 - 1 minimizers in one sketch");
  int thr = INT_MAX;
  int64_t dropped = 0;
  DevBuf<uint32_t> sorted_hash, uniq, counts, num_runs;
  if (N > 0) {
    hipStream_t st = s->stream.get();
    DevBuf<unsigned char> temp;
    DevBuf<size_t> n_selected;
    sorted_hash.ensure((size_t)N); uniq.ensure((size_t)N); counts.ensure((size_t)N); num_runs.ensure(1); n_selected.ensure(1);
    with_temp(temp, [&](void *t, size_t &bytes) { return rocprim::radix_sort_keys(t, bytes, s->rec.hash.p, sorted_hash.p, (size_t)N, 0u, 32u, st); });
    with_temp(temp, [&](void *t, size_t &bytes) {
      return rocprim::run_length_encode(t, bytes, sorted_hash.p, (size_t)N, uniq.p, counts.p, num_runs.p, st);
    });
    uint32_t U = 0;
    num_runs.download(&U, 1, st);
    FA_HIP(hipStreamSynchronize(st));
    thr = frequency_threshold(counts.p, (int64_t)U, temp, st);
    if (thr < INT_MAX) {
      // the distinct hashes ascend, and so do the ones kept; the sorted copy has served and takes them
      with_temp(temp, [&](void *t, size_t &bytes) {
        return rocprim::select(t, bytes, uniq.p, rocprim::make_transform_iterator(counts.p, ListAtLeast{(uint32_t)thr}), sorted_hash.p, n_selected.p,
                               (size_t)U, st);
      });
      size_t kept = 0;
      n_selected.download(&kept, 1, st);
      FA_HIP(hipStreamSynchronize(st));
      dropped = (int64_t)kept;
    }
    if (dropped > cap) {
      *n_drop = dropped;
      FA_REQUIRE(false, FA_ERR_INVALID, "destination holds fewer keys than reach the threshold (*n_drop is what it takes)");
    }
    if (dropped > 0) {
      FA_HIP(hipMemcpyAsync(d_drop_keys, sorted_hash.p, (size_t)dropped * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      FA_HIP(hipStreamSynchronize(st));
    }
  }
  *threshold = thr;
  *n_drop = dropped;
}
