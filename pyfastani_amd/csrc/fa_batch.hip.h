// fa_batch.hip.h -- fa_genomes: packed query genomes resident in HBM, cut into fragments and tiles, and their upload from
// host buffers, FASTA files or files packed once (fa_packed).  Host side of the one translation unit fa_engine.hip;
// fa_genomes and fa_packed are the C ABI's opaque types, hence the global namespace.
#pragma once

#include <atomic>
#include <chrono>
#include <shared_mutex>
#include <vector>

#include "fa_common.h"
#include "fa_fasta.h"
#include "fa_index.hip.h"
#include "fa_ingest.h"

using namespace fa;

// Everything the kernels read of a batch sits in ONE device allocation, filled by ONE host-to-device copy from a staging
// image of the same layout (BatchLayout, fa_ingest.h).  Only the exception lists (rare: N runs, IUPAC codes) are separate.
struct fa_genomes {
  fa_params P;
  DevBuf<unsigned char> blob;
  DevBuf<int64_t> exc_pos;
  DevBuf<uint8_t> exc_val;
  StoreView store;                          // pointers into blob / the exception buffers
  const Tile *tiles = nullptr;
  const int32_t *d_frag_tile_lo = nullptr, *d_frag_query = nullptr, *d_frag_qseq = nullptr, *d_total_frag = nullptr;
  int32_t n_genomes = 0;
  std::vector<int64_t> genome_frag_lo;      // [n_genomes + 1] fragment range of each genome
  std::vector<int32_t> frag_tile_lo;        // [F + 1]
  std::vector<int64_t> contig_frag_lo;      // first fragment of every contig that holds fragments (ascending)
  std::vector<uint64_t> total_fragments, total_length;
  std::vector<int32_t> n_short;
  int64_t F = 0, ntiles = 0;
  uint64_t total_bases = 0;                 // bases inside fragments
  std::vector<unsigned char, NoInitAlloc<unsigned char>> host_image;   // staging image when no pinned buffer is supplied (every byte of it is written: no zero fill)
  PinnedBuf pin_image;                      // staging image of a batch that is refilled (fa_genomes_reload_fasta)
  Stream up_stream;                         // FASTA uploads run on the batch's own stream
  // a failed refill leaves an empty (but valid) batch
  void reset_empty() {
    n_genomes = 0; F = 0; ntiles = 0;
    genome_frag_lo.assign(1, 0); total_fragments.clear(); total_length.clear(); n_short.clear();
  }
  uint64_t serial = 0;                      // a new number for every upload (caches keyed on a batch compare this, not its address)
};
static std::atomic<uint64_t> g_batch_serial{0};

// pack + cut into fragments + tiles + upload, in place: `g` may be a batch object whose device buffers are recycled, contents
// replaced.  That and `pin` (pinned staging memory the image is built in, so that the one upload is a plain DMA) serve the
// one-query-at-a-time call; without `pin` the image is built in pageable memory.
// `packed` (fa_genomes_upload_fasta): contig c is record packed[c] of a file that read_fasta_packed has packed already -- its
// words are copied where `contigs` would be packed; `contigs` is not read then.
// `sync_pinned` (fa_genomes_reload_fasta: device buffers, pinned image and upload stream are recycled from chunk to chunk): wait
// for the upload although the image is pinned (the image is reused next).
static void fill_genomes(fa_genomes *g, const fa_params &P, hipStream_t st, const void *const *contigs, const int64_t *lengths,
                         const int32_t *contig_genome, int64_t n_contigs, int32_t n_genomes, int width,
                         float *host_ms, PinnedBuf *pin, const PackedRef *packed, bool sync_pinned) {
  require_device();
  const auto t_begin = std::chrono::steady_clock::now();
  auto lap = [&, last = t_begin](int slot) mutable {
    const auto now = std::chrono::steady_clock::now();
    if (host_ms) host_ms[slot] = std::chrono::duration<float, std::milli>(now - last).count();
    last = now;
  };
  FA_REQUIRE(width == 1 || width == 2 || width == 4, FA_ERR_INVALID, "char_width must be 1, 2 or 4");
  g->P = P;
  g->serial = ++g_batch_serial;
  // which contigs are mapped, how many whole fragments each holds, the per-genome counters and every size of the image
  BatchPlan plan = plan_batch(P, lengths, contig_genome, n_contigs, n_genomes, TILE, sizeof(Tile));
  const BatchLayout &at = plan.at;
  const int64_t F = plan.F, ntiles = plan.ntiles, tiles_per_frag = plan.tiles_per_frag;
  const int frag = P.fragment_length;
  g->n_genomes = n_genomes;
  g->F = F; g->ntiles = ntiles; g->total_bases = plan.total_bases;
  g->genome_frag_lo = std::move(plan.genome_frag_lo); g->contig_frag_lo = std::move(plan.contig_frag_lo);
  g->total_fragments = std::move(plan.total_fragments); g->total_length = std::move(plan.total_length); g->n_short = std::move(plan.n_short);
  HostStore hs;
  hs.protein = P.alphabet_size != 4;
  const size_t image_bytes = at.image_bytes, bases = plan.bases;
  unsigned char *img;
  if (pin) { pin->ensure(image_bytes); img = pin->p; }
  else { g->host_image.resize(image_bytes); img = g->host_image.data(); }
  StageTrace tr("upload_genomes");
  // the slack behind the packed words / bytes (the sketch kernel's funnel shift reads one word past the end)
  if (!hs.protein) memset(img + at.packed.at + bases / 4, 0, at.packed.bytes - bases / 4); else memset(img + at.bytes.at + bases, 0, at.bytes.bytes - bases);
  if (packed) {
    std::vector<PackedRef> use_ref;
    for (const ContigJob &cj : plan.jobs) use_ref.push_back(PackedRef{packed[cj.c].file, packed[cj.c].rec, cj.nfrag * frag});
    place_packed(hs, use_ref.data(), (int64_t)use_ref.size(), (uint32_t *)(img + at.packed.at), img + at.bytes.at);
  } else {
    std::vector<const void *> use_ptr;
    for (const ContigJob &cj : plan.jobs) use_ptr.push_back(contigs[cj.c]);
    hs.pack_many(use_ptr.data(), plan.use_len.data(), (int64_t)use_ptr.size(), width, (uint32_t *)(img + at.packed.at), img + at.bytes.at);
  }
  tr.mark("pack", st);
  lap(0);
  // fragments and tiles, written straight into the image by the host pool (1.7 M fragments and 5 M tiles for a thousand
  // genomes were one thread's loop)
  Tile *tiles = (Tile *)(img + at.tiles.at);
  int32_t *frag_query = (int32_t *)(img + at.frag_query.at), *frag_qseq = (int32_t *)(img + at.frag_qseq.at), *tf = (int32_t *)(img + at.total_frag.at);
  g->frag_tile_lo.assign((size_t)F + 1, 0);
  HostPool::get().parallel_for(plan.jobs.size(), [&](size_t j) {
    const ContigJob &cj = plan.jobs[j];
    for (int64_t i = 0; i < cj.nfrag; i++) {
      const int64_t f = cj.nf0 + i;
      g->frag_tile_lo[(size_t)f] = (int32_t)(f * tiles_per_frag);
      make_tiles_at(tiles + f * tiles_per_frag, hs, hs.seq_off[cj.si] + i * frag, frag, (int)f, P.kmer_size, P.window_size);
      frag_qseq[f] = (int32_t)(cj.q0 + i);
      frag_query[f] = cj.gi;
    }
  });
  g->frag_tile_lo[(size_t)F] = (int32_t)ntiles;
  memcpy(img + at.frag_tile_lo.at, g->frag_tile_lo.data(), ((size_t)F + 1) * 4);
  for (int i = 0; i < n_genomes; i++) tf[i] = (int32_t)g->total_fragments[i];
  tr.mark("fragments_tiles", st);
  lap(1);
  g->blob.ensure(image_bytes);
  // The one-query call (image in the workspace's pinned block, untouched until the call returns): the sketch stage reads the
  // packed words STRAIGHT from the pinned image over PCIe -- every word is read once, by the workgroup that hashes it, and the
  // kernel is bound by its hashing, so the 1.25 MB travel inside its 67 us instead of in a 28 us copy in front of it; only the
  // tile and fragment tables (read by every stage) are copied.  FA_QUERY_ZERO_COPY=0: the whole image is copied.
  const bool zero_copy = knob::query_zero_copy() != 0 && pin && !sync_pinned && !hs.protein;
  if (zero_copy) FA_HIP(hipMemcpyAsync(g->blob.p + at.tiles.at, img + at.tiles.at, image_bytes - at.tiles.at, hipMemcpyHostToDevice, st));
  else FA_HIP(hipMemcpyAsync(g->blob.p, img, image_bytes, hipMemcpyHostToDevice, st));
  const int64_t n_exc = (int64_t)hs.exc_pos.size();
  if (n_exc) { g->exc_pos.upload(hs.exc_pos, st); g->exc_val.upload(hs.exc_val, st); }
  g->store = StoreView();
  g->store.packed = hs.protein ? nullptr : (const uint32_t *)((zero_copy ? img : g->blob.p) + at.packed.at);
  g->store.bytes = hs.protein ? (const uint8_t *)(g->blob.p + at.bytes.at) : nullptr;
  g->store.exc_pos = g->exc_pos.p; g->store.exc_val = g->exc_val.p; g->store.n_exc = n_exc;
  g->tiles = (const Tile *)(g->blob.p + at.tiles.at);
  g->d_frag_tile_lo = (const int32_t *)(g->blob.p + at.frag_tile_lo.at);
  // the CGI bins of a pass are indexed by the genome number relative to the first genome of the pass; passes start at
  // genome boundaries, so the per-fragment genome numbers are batch-wide and the kernel subtracts the pass's first genome
  g->d_frag_query = (const int32_t *)(g->blob.p + at.frag_query.at);
  g->d_frag_qseq = (const int32_t *)(g->blob.p + at.frag_qseq.at);
  g->d_total_frag = (const int32_t *)(g->blob.p + at.total_frag.at);
  // the staging image must stay untouched until the copy has left it (pageable copies return after staging, pinned ones
  // are asynchronous).  An image in the caller's pinned block (the one-query call: the block belongs to the workspace and
  // is not touched again before the call returns, and the pass runs on this same stream, behind the copy) needs no
  // synchronisation; otherwise one per upload
  if (!pin || sync_pinned) {
    FA_HIP(hipStreamSynchronize(st));
    std::vector<unsigned char, NoInitAlloc<unsigned char>>().swap(g->host_image);
  }
  tr.mark("uploads", st);
  lap(2);
}

// the records of packed files as one contig list, one genome per file
struct PackedContigs {
  std::vector<PackedRef> refs;
  std::vector<int64_t> lens;
  std::vector<int32_t> genome;
  PackedContigs(const PackedFasta *files, int32_t n_paths) {
    for (int32_t i = 0; i < n_paths; i++)
      for (size_t r = 0; r < files[i].rec_len.size(); r++) { refs.push_back(PackedRef{&files[i], (int64_t)r, files[i].rec_len[r]}); lens.push_back(files[i].rec_len[r]); genome.push_back(i); }
  }
};
// one genome per FASTA file, every file read + packed by its own task of the host pool (read_fasta_packed_many), then the
// batch image assembled from the packed records and uploaded on the batch's own stream
// genomes [first, first + count) of files packed already (one genome per file) as the batch `g`
static void fill_genomes_from_packed(fa_mapper *m, fa_genomes *g, const PackedFasta *files, int32_t n_paths, bool pinned) {
  const PackedContigs all(files, n_paths);
  bind_device(m->device);
  // (its own stream: a batch may be uploaded while another thread maps the previous one, Mapper.query_fasta_stream)
  fill_genomes(g, m->P, g->up_stream.get(hipStreamNonBlocking), nullptr, all.lens.data(), all.genome.data(), (int64_t)all.refs.size(), n_paths, 1, nullptr,
               pinned ? &g->pin_image : nullptr, all.refs.data(), true);
}
static void fill_genomes_from_fasta(fa_mapper *m, fa_genomes *g, const char *const *paths, int32_t n_paths, bool pinned) {
  std::vector<PackedFasta> files;
  read_fasta_packed_many(paths, (size_t)n_paths, m->P.alphabet_size != 4, files);
  fill_genomes_from_packed(m, g, files.data(), n_paths, pinned);
}

// FASTA files read and packed ONCE, to be used as references AND as queries (an all-vs-all reads every file one time)
struct fa_packed {
  bool protein = false;
  std::vector<PackedFasta> files;
  // fa_packed_append grows `files` (and moves every PackedFasta) under the exclusive lock; the calls that read them
  // (fa_packed_info, fa_sketch_add_packed, fa_genomes_reload_packed -- all run without the GIL) hold it shared for their duration
  std::shared_mutex mtx;
};
