// fa_refsketch.hip.h -- fa_sketch: reference genomes being collected (skch::Sketch + pyfastani's counters), the flush
// that sketches the pending contigs on the device, and the saved state going in.  Host side of the one translation unit
// fa_engine.hip; fa_sketch is the C ABI's opaque type, hence the global namespace.
#pragma once

#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>

#include "fa_batch.hip.h"
#include "fa_common.h"
#include "fa_ingest.h"
#include "fa_k1.hip.h"

using namespace fa;

// the minimizer records of a sketch: three parallel device arrays that grow, fill and empty together
struct RecArrays {
  DevBuf<uint32_t> hash;
  DevBuf<int32_t> seq, wpos;
  // room for n records, the first `keep` of them preserved
  void reserve(size_t n, size_t keep, hipStream_t st) { hash.ensure(n, true, st, keep); seq.ensure(n, true, st, keep); wpos.ensure(n, true, st, keep); }
  // n records from host (hipMemcpyHostToDevice) or device memory replace the content
  void load(const uint32_t *h, const int32_t *s, const int32_t *w, size_t n, hipMemcpyKind kind, hipStream_t st) {
    hash.ensure(n); seq.ensure(n); wpos.ensure(n);
    copy(hash.p, seq.p, wpos.p, h, s, w, n, kind, st);
  }
  // the first n records to host (hipMemcpyDeviceToHost) or device memory
  void store(uint32_t *h, int32_t *s, int32_t *w, size_t n, hipMemcpyKind kind, hipStream_t st) const { copy(h, s, w, hash.p, seq.p, wpos.p, n, kind, st); }
  static void copy(uint32_t *dh, int32_t *ds, int32_t *dw, const uint32_t *h, const int32_t *s, const int32_t *w, size_t n, hipMemcpyKind kind, hipStream_t st) {
    if (!n) return;
    FA_HIP(hipMemcpyAsync(dh, h, n * sizeof(uint32_t), kind, st));
    FA_HIP(hipMemcpyAsync(ds, s, n * sizeof(int32_t), kind, st));
    FA_HIP(hipMemcpyAsync(dw, w, n * sizeof(int32_t), kind, st));
  }
};

struct fa_sketch {
  fa_params P;
  int device = -1;
  Stream stream;
  Stream up_stream;                       // uploads of a flush (the next chunk's sequence while this one is hashed)
  HostStore pending;                      // packed contigs not yet sketched
  RefBook book;                           // the genomes' counters, and the contig id of each pending sequence (fa_ingest.h)
  RecArrays rec;
  int64_t nrec = 0;
  SketchWork work;
  std::mutex mtx;

  void reset_data() {
    pending.clear(); pending.protein = P.alphabet_size != 4;
    book.reset(); nrec = 0;
  }

  // sketch every pending contig on the device and append the records
  void flush() {
    if (pending.seq_off.empty()) return;
    require_device();
    bind_device(device);
    stream.get();
    StageTrace tr("sketch flush");
    // the packed sequence goes up chunk by chunk on a stream of its own: the copy of chunk c + 1 (a staged copy from pageable
    // memory: the host thread is inside it) runs while the device hashes chunk c -- 25-50 ms of a thousand genomes' 90-110
    up_stream.get();
    DevStore store;
    store.begin(pending, stream);
    const int64_t nseq_all = (int64_t)pending.seq_off.size();
    // staging is 8 B per k-mer position; a chunk takes an eighth of the free HBM at most, between 96 M positions (768 MiB) and
    // 512 M (4 GiB: a thousand genomes are ten chunks, not fifty-two with two synchronisations each -- and not two chunks whose
    // 34 GB of staging a fresh process has to map first)
    size_t hbm_free = 0, hbm_total = 0;
    if (hipMemGetInfo(&hbm_free, &hbm_total) != hipSuccess) { (void)hipGetLastError(); hbm_free = 0; }
    const int64_t chunk_positions = std::max<int64_t>(96LL << 20, std::min<int64_t>((int64_t)(hbm_free / 8 / 8), 512LL << 20));
    // the records are appended chunk by chunk: reserve for all of them once (2 / (w + 1) of the positions are minimizers, a
    // quarter of headroom; `ensure(keep)` below still grows the arrays if a sequence is denser) instead of regrowing -- and
    // copying -- them a dozen times
    {
      int64_t positions_all = 0;
      for (int64_t q = 0; q < nseq_all; q++) positions_all += pending.seq_len[q];
      const double per_pos = P.alphabet_size == 4 ? 2.0 / (P.window_size + 1) : 1.0;
      const size_t expect = (size_t)nrec + (size_t)((double)positions_all * std::min(1.0, per_pos * 1.25)) + 1024;
      rec.reserve(expect, (size_t)nrec, stream);
    }
    // chunk boundaries first (the copy of the next chunk is issued while this one is hashed)
    std::vector<int64_t> cuts{0};
    for (int64_t q = 0, positions = 0; q < nseq_all; q++) {
      if (q > cuts.back() && positions + pending.seq_len[q] > chunk_positions) { cuts.push_back(q); positions = 0; }
      positions += pending.seq_len[q];
    }
    cuts.push_back(nseq_all);
    auto base_of = [&](int64_t q) { return q < nseq_all ? pending.seq_off[(size_t)q] : pending.total; };
    std::vector<Event> sent(cuts.size() - 1);
    auto send = [&](size_t c) {
      store.upload_bases(pending, base_of(cuts[c]), base_of(cuts[c + 1]), up_stream);
      FA_HIP(hipEventRecord(sent[c].get(hipEventDisableTiming), up_stream));
    };
    FA_HIP(hipStreamSynchronize(stream));           // (the buffers of `begin` exist before the other stream writes them)
    send(0);
    tr.mark("upload", up_stream);
    DevBuf<int32_t> d_seq_tile_lo, d_drop, d_drop_off, d_seq_ids;
    for (size_t chunk = 0; chunk + 1 < cuts.size(); chunk++) {
      const int64_t s0 = cuts[chunk], s1 = cuts[chunk + 1];
      std::vector<Tile> tiles;
      std::vector<int32_t> seq_tile_lo, seq_ids;
      // (tiles whose positions + halo are whole hashing trips: k1_tile_len)
      const int tile_len = k1_tile_len(P.window_size);
      // (five million tiles for a thousand genomes: counted first, then filled by the host pool -- 91 ms of one thread before)
      int64_t tile_total = 0;
      for (int64_t q = s0; q < s1; q++) {
        seq_tile_lo.push_back((int32_t)tile_total);
        tile_total += tile_count(pending.seq_len[q], P.kmer_size, tile_len);
        seq_ids.push_back(book.pending_contig[q]);
      }
      seq_tile_lo.push_back((int32_t)tile_total);
      FA_REQUIRE(tile_total < (1LL << 31) - 1, FA_ERR_UNSUPPORTED, "too many tiles in one sketch chunk");
      tiles.resize((size_t)tile_total);
      {
        const int64_t nq = s1 - s0, per = std::max<int64_t>(1, nq / 512);       // (a few hundred tasks at most)
        HostPool::get().parallel_for((size_t)((nq + per - 1) / per), [&](size_t t) {
          for (int64_t q = s0 + (int64_t)t * per; q < std::min(s1, s0 + ((int64_t)t + 1) * per); q++)
            make_tiles_at(tiles.data() + seq_tile_lo[(size_t)(q - s0)], pending, pending.seq_off[q], pending.seq_len[q], (int)(q - s0), P.kmer_size, P.window_size, tile_len);
        });
      }
      const int nseq = (int)(s1 - s0), ntiles = (int)tiles.size();
      tr.mark("host_tiles", stream);
      if (ntiles > 0) {
        work.tiles.upload(tiles, stream);
        work.reserve((size_t)ntiles);
        work.tile_off.ensure(ntiles + 1);
        FA_HIP(hipMemsetAsync(work.tile_count.p + ntiles, 0, sizeof(int32_t), stream));
        tr.mark("alloc_tiles", stream);
        FA_HIP(hipStreamWaitEvent(stream, sent[chunk], 0));
        launch_sketch_tiles(P, store.view(), work.tiles.p, ntiles, work.stage_hash.p, work.stage_wpos.p, work.tile_count.p, stream);
        if (chunk + 2 < cuts.size()) send(chunk + 1);          // (behind the launch: the host copies while the device hashes)
        tr.mark("k_sketch", stream);
        d_seq_tile_lo.upload(seq_tile_lo, stream);
        d_seq_ids.upload(seq_ids, stream);
        d_drop.ensure(nseq + 1);
        d_drop_off.ensure(nseq + 1);
        FA_HIP(hipMemsetAsync(d_drop.p + nseq, 0, sizeof(int32_t), stream));
        hipLaunchKernelGGL(k_suppress_runs, dim3(ceil_div(nseq, 128)), dim3(128), 0, stream, d_seq_tile_lo.p, nseq,
                           work.tile_count.p, work.stage_hash.p, work.stage_wpos.p, d_drop.p);
        exclusive_sum_i32(work.cub_temp, work.tile_count.p, work.tile_off.p, ntiles + 1, stream);
        exclusive_sum_i32(work.cub_temp, d_drop.p, d_drop_off.p, nseq + 1, stream);
        int32_t total = 0, dropped = 0;
        FA_HIP(hipMemcpyAsync(&total, work.tile_off.p + ntiles, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        FA_HIP(hipMemcpyAsync(&dropped, d_drop_off.p + nseq, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        FA_HIP(hipStreamSynchronize(stream));
        const int64_t nout = (int64_t)total - dropped;
        tr.mark("scan", stream);
        rec.reserve((size_t)(nrec + nout), (size_t)nrec, stream);
        tr.mark("grow", stream);
        hipLaunchKernelGGL(k_compact_records, dim3(ntiles), dim3(256), 0, stream, work.tiles.p, work.tile_count.p,
                           work.tile_off.p, d_seq_tile_lo.p, d_drop.p, d_drop_off.p, work.stage_hash.p, work.stage_wpos.p,
                           d_seq_ids.p, nrec, rec.hash.p, rec.seq.p, rec.wpos.p);
        FA_HIP(hipGetLastError());
        FA_HIP(hipStreamSynchronize(stream));
        tr.mark("compact", stream);
        nrec += nout;
      } else if (chunk + 2 < cuts.size()) send(chunk + 1);
    }
    FA_HIP(hipStreamSynchronize(up_stream));
    pending.clear();
    pending.protein = P.alphabet_size != 4;
    book.pending_contig.clear();
  }
};

// the saved state of a sketch replaces its content; the records come from host (hipMemcpyHostToDevice) or device memory
static void sketch_set_state(fa_sketch *s, int64_t n_genomes, const uint64_t *lengths, const int32_t *sbf, int64_t counter, int64_t n_min,
                             const uint32_t *hash, const int32_t *seq_id, const int32_t *wpos, hipMemcpyKind kind) {
  std::lock_guard<std::mutex> lock(s->mtx);
  bind_device(s->device);
  FA_REQUIRE(n_min >= 0 && n_genomes >= 0, FA_ERR_INVALID, "negative count");
  s->reset_data();
  s->book.lengths.assign(lengths, lengths + n_genomes);
  s->book.seqs_by_file.assign(sbf, sbf + n_genomes);
  s->book.counter = counter;
  if (n_min > 0) {
    require_device();
    bind_device(s->device);
    s->rec.load(hash, seq_id, wpos, (size_t)n_min, kind, s->stream.get());
    FA_HIP(hipStreamSynchronize(s->stream));
  }
  s->nrec = n_min;
}

// the bookkeeping of fa_sketch_add_fasta_many over files that are packed already (s->mtx held by the caller)
static void sketch_add_packed_files(fa_sketch *s, const PackedFasta *files, int32_t n_paths, int64_t *n_records, int64_t *n_short) {
  const PackedContigs all(files, n_paths);
  std::vector<PackedRef> refs;
  RefStage add(s->book, OpenGenome::REFUSE, n_paths);
  add.genomes(s->P, all.lens.data(), all.genome.data(), (int64_t)all.refs.size(), n_paths, [&](int64_t c) { refs.push_back(all.refs[(size_t)c]); });
  add.commit(s->book, [&] { if (!refs.empty()) append_packed(s->pending, refs.data(), (int64_t)refs.size()); });
  for (int32_t i = 0; i < n_paths; i++) {
    if (n_records) n_records[i] = (int64_t)files[i].rec_len.size();
    if (n_short) n_short[i] = add.n_short[(size_t)i];
  }
}

// fa_sketch_index: the records of the sketch become an index (build_index); the sketch is emptied
static void sketch_index(fa_sketch *s, fa_mapper **out) {
  std::lock_guard<std::mutex> lock(s->mtx);
  bind_device(s->device);
  require_device();
  s->flush();
  bind_device(s->device);
  std::unique_ptr<fa_mapper> m(new fa_mapper());
  m->P = s->P;
  m->device = s->device;
  if (m->device < 0) FA_HIP(hipGetDevice(&m->device));
  m->stream.get();
  m->N = s->nrec;
  s->rec.reserve((size_t)m->N + 4, (size_t)m->N, m->stream);
  m->rec_hash = std::move(s->rec.hash); m->rec_seq = std::move(s->rec.seq); m->rec_wpos = std::move(s->rec.wpos);
  m->lengths = s->book.lengths;
  m->seqs_by_file = s->book.seqs_by_file;
  if (!m->seqs_by_file.empty() && m->seqs_by_file.back() < (int32_t)s->book.counter) {
    // contigs added after the last end_genome belong to no genome; keep the tables consistent
    m->seqs_by_file.back() = (int32_t)s->book.counter;
  }
  build_index(*m);
  s->reset_data();                                     // _fastani.pyx:803-804
  *out = m.release();
}

// fa_debug_sketch_sequence: one sequence through a sketch of its own; the records in position order
static void debug_sketch_sequence(const fa_params *params, const void *data, int64_t length, int char_width, uint32_t *hash,
                                  int32_t *wpos, int64_t cap, int64_t *n) {
  fa_sketch s;
  s.P = *params;
  s.reset_data();
  if (length >= params->kmer_size) {
    s.pending.append(data, char_width, length);
    s.book.pending_contig.push_back(0);
  }
  s.flush();
  *n = s.nrec;
  size_t c = (size_t)std::min<int64_t>(s.nrec, cap);
  if (c) {
    s.rec.hash.download(hash, c, s.stream);
    s.rec.wpos.download(wpos, c, s.stream);
    FA_HIP(hipStreamSynchronize(s.stream));
  }
}
