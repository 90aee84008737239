// fa_engine.hip -- the C ABI of libfastani_hip.so (include/fastani_hip.h): the error guard, parameter validation and the
// entry points, each a call into the object it belongs to.  One header per object: the K1 launcher (fa_k1.hip.h), the
// reference sketch (fa_refsketch.hip.h), the resident batch (fa_batch.hip.h), the index and its workspaces
// (fa_index.hip.h), the query pass (fa_query.hip.h), the selection drivers (fa_select.hip.h), the signatures of a resident
// batch (fa_batchsig.hip.h) and the reductions over finished results (fa_reduce.hip.h).  All of it is this one translation unit.
// There is no CPU fallback anywhere in the library: without a HIP device every compute entry point fails.
#include <cstring>   // (before rocPRIM, whose texture_cache_iterator.hpp calls memset without including it)

#include <cmath>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "fa_batch.hip.h"
#include "fa_batchsig.hip.h"
#include "fa_common.h"
#include "fa_fasta.h"
#include "fa_index.hip.h"
#include "fa_query.hip.h"
#include "fa_reduce.hip.h"
#include "fa_refsketch.hip.h"
#include "fa_select.hip.h"
#include "fa_stats.h"

using namespace fa;

// ------------------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

template <typename F>
static int guarded(F &&fn) {
  try {
    fn();
    return FA_OK;
  } catch (const Error &e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::bad_alloc &) {
    g_last_error = "host allocation failed";
    return FA_ERR_NOMEM;
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return FA_ERR_INTERNAL;
  }
}

static void validate_params(const fa_params &p) {
  FA_REQUIRE(p.kmer_size >= 1 && p.kmer_size <= 2048, FA_ERR_INVALID, "kmer_size must be in [1, 2048]");
  FA_REQUIRE(p.fragment_length >= 1, FA_ERR_INVALID, "fragment_length must be strictly positive");
  FA_REQUIRE(p.window_size >= 1, FA_ERR_INVALID, "window_size must be strictly positive");
  FA_REQUIRE(p.alphabet_size == 4 || p.alphabet_size == 20, FA_ERR_INVALID, "alphabet_size must be 4 or 20");
  FA_REQUIRE(sketch_layout(p.kmer_size, p.window_size).total <= 160 * 1024, FA_ERR_UNSUPPORTED,
             "window_size/kmer_size too large for the LDS-staged sketch kernel (tile + 2w + k must fit 160 KiB)");
}

extern "C" {

const char *fa_last_error(void) { return g_last_error.c_str(); }
int fa_version(void) { return 100; }
int fa_device_trim(uint64_t *held_bytes) {
  return guarded([&] {
    if (held_bytes) *held_bytes = (uint64_t)DevPool::get().held();
    DevPool::get().trim();
  });
}

int fa_device_count(int *count) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
  *count = n;
  return FA_OK;
}
int fa_set_device(int device) {
  return guarded([&] { require_device(); FA_HIP(hipSetDevice(device)); g_device.store(device); });
}

int fa_recommended_window_size(double p_value, int k, int alphabet_size, float identity, int fragment_length,
                               uint64_t reference_size, int *window) {
  return guarded([&] { *window = stat_recommended_window(p_value, k, alphabet_size, identity, fragment_length, reference_size); });
}
int fa_estimate_minimum_hits_relaxed(int s, int k, float identity, int *hits) {
  return guarded([&] { *hits = stat_min_hits_relaxed(s, k, identity); });
}
int fa_mapping_identity(int shared, int s, int k, float *identity, float *upper) {
  return guarded([&] { FA_REQUIRE(s > 0, FA_ERR_INVALID, "sketch_size must be positive"); stat_identity(shared, s, k, identity, upper); });
}

// host twin of the device hash (same published algorithm as fa_sketch.hip.h's Murmur)
uint32_t fa_hash(const void *kmer, int len) {
  const uint8_t *d = (const uint8_t *)kmer;
  auto rotl = [](uint64_t x, int r) { return (x << r) | (x >> (64 - r)); };
  auto fmix = [](uint64_t k) { k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33; return k; };
  const uint64_t c1 = 0x87c37b91114253d5ULL, c2 = 0x4cf5ad432745937fULL;
  uint64_t h1 = 42, h2 = 42;
  int nb = len / 16;
  for (int i = 0; i < nb; i++) {
    uint64_t k1, k2;
    memcpy(&k1, d + 16 * i, 8); memcpy(&k2, d + 16 * i + 8, 8);
    k1 *= c1; k1 = rotl(k1, 31); k1 *= c2; h1 ^= k1; h1 = rotl(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
    k2 *= c2; k2 = rotl(k2, 33); k2 *= c1; h2 ^= k2; h2 = rotl(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
  }
  const uint8_t *t = d + 16 * nb;
  int rem = len & 15;
  uint64_t k1 = 0, k2 = 0;
  for (int j = 0; j < rem; j++) { if (j < 8) k1 |= (uint64_t)t[j] << (8 * j); else k2 |= (uint64_t)t[j] << (8 * (j - 8)); }
  if (rem > 8) { k2 *= c2; k2 = rotl(k2, 33); k2 *= c1; h2 ^= k2; }
  if (rem > 0) { k1 *= c1; k1 = rotl(k1, 31); k1 *= c2; h1 ^= k1; }
  h1 ^= (uint64_t)len; h2 ^= (uint64_t)len; h1 += h2; h2 += h1; h1 = fmix(h1); h2 = fmix(h2);
  return (uint32_t)(h1 + h2);
}

int fa_sketch_new(const fa_params *params, fa_sketch **out) {
  return guarded([&] {
    validate_params(*params);
    std::unique_ptr<fa_sketch> s(new fa_sketch());
    s->P = *params;
    s->device = g_device.load();
    s->reset_data();
    *out = s.release();
  });
}
void fa_sketch_free(fa_sketch *s) { delete s; }
int fa_sketch_add_contig(fa_sketch *s, const void *data, int64_t length, int char_width, int *added) {
  return guarded([&] {
    FA_REQUIRE(char_width == 1 || char_width == 2 || char_width == 4, FA_ERR_INVALID, "char_width must be 1, 2 or 4");
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    RefStage add(s->book, OpenGenome::FOLD);
    const bool ok = add.contig(s->P, length);
    add.commit(s->book, [&] { if (ok) s->pending.append(data, char_width, length); });
    if (added) *added = ok ? 1 : 0;
  });
}
struct fa_fasta { FastaFile f; };
int fa_fasta_open(const char *path, fa_fasta **out) {
  return guarded([&] {
    FA_REQUIRE(path && out, FA_ERR_INVALID, "null argument");
    std::unique_ptr<fa_fasta> h(new fa_fasta());
    h->f.open(path);
    *out = h.release();
  });
}
int fa_fasta_next(fa_fasta *f, int *has_record, const char **id, int64_t *id_length, const unsigned char **seq, int64_t *seq_length) {
  return guarded([&] {
    const bool ok = f->f.next();
    *has_record = ok ? 1 : 0;
    if (!ok) return;
    *id = f->f.id.data(); *id_length = (int64_t)f->f.id.size();
    *seq = f->f.seq.data(); *seq_length = (int64_t)f->f.seq.size();
  });
}
void fa_fasta_close(fa_fasta *f) { delete f; }

int fa_sketch_add_fasta(fa_sketch *s, const char *path, int64_t *n_records, int64_t *n_short) {
  return guarded([&] {
    FA_REQUIRE(path, FA_ERR_INVALID, "null path");
    std::vector<FastaSeq> seqs;
    read_fasta_records(path, seqs);
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    std::vector<const void *> ptrs;
    std::vector<int64_t> all, lens;
    for (auto &q : seqs) all.push_back((int64_t)q.size);
    RefStage add(s->book, OpenGenome::FOLD);
    add.genomes(s->P, all.data(), nullptr, (int64_t)all.size(), 1, [&](int64_t c) { ptrs.push_back(seqs[(size_t)c].data.get()); lens.push_back(all[(size_t)c]); });
    add.commit(s->book, [&] { if (!ptrs.empty()) s->pending.append_many(ptrs.data(), lens.data(), (int64_t)ptrs.size(), 1); });
    if (n_records) *n_records = (int64_t)seqs.size();
    if (n_short) *n_short = add.n_short[0];
  });
}
// Many reference genomes at once from host buffers: contig c belongs to genome contig_genome[c] (non-decreasing); the effect of
// n_genomes x (fa_sketch_add_contig per contig, fa_sketch_end_genome) with ONE call of the packer over all contigs -- the
// per-genome calls wake the host pool a thousand times for a thousand genomes (0.4-0.5 s of `host_pack_s` on config 3).
int fa_sketch_add_genomes(fa_sketch *s, const void *const *contigs, const int64_t *lengths, const int32_t *contig_genome, int64_t n_contigs,
                          int32_t n_genomes, int char_width, int32_t *n_short) {
  return guarded([&] {
    FA_REQUIRE(char_width == 1 || char_width == 2 || char_width == 4, FA_ERR_INVALID, "char_width must be 1, 2 or 4");
    FA_REQUIRE(n_contigs >= 0 && n_genomes >= 0 && (n_contigs == 0 || (contigs && lengths && contig_genome)), FA_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    std::vector<const void *> ptrs;
    std::vector<int64_t> lens;
    RefStage add(s->book, OpenGenome::REFUSE, n_genomes);
    add.genomes(s->P, lengths, contig_genome, n_contigs, n_genomes, [&](int64_t c) { ptrs.push_back(contigs[c]); lens.push_back(lengths[c]); });
    add.commit(s->book, [&] { if (!ptrs.empty()) s->pending.append_many(ptrs.data(), lens.data(), (int64_t)ptrs.size(), char_width); });
    if (n_short) for (int32_t i = 0; i < n_genomes; i++) n_short[i] = (int32_t)add.n_short[(size_t)i];
  });
}
// Many reference genomes at once, one per FASTA file, in the order given: the files are read and packed concurrently (one
// task per file), then appended to the pending store exactly as fa_sketch_add_fasta would have added them one by one.
int fa_sketch_add_fasta_many(fa_sketch *s, const char *const *paths, int32_t n_paths, int64_t *n_records, int64_t *n_short) {
  return guarded([&] {
    FA_REQUIRE(paths && n_paths >= 0, FA_ERR_INVALID, "null paths or negative count");
    StageTrace tr("add_fasta_many");
    std::vector<PackedFasta> files;
    read_fasta_packed_many(paths, (size_t)n_paths, s->P.alphabet_size != 4, files);
    tr.mark("read_pack", nullptr);
    if (tr.on) {
      FastaTaskClock &c = fasta_task_clock();
      fprintf(stderr, "[fa trace] fasta tasks so far: %llu files, per-task sums: read %.1f ms, record search %.1f ms, pack %.1f ms\n", (unsigned long long)c.files.load(),
              c.read_ns.load() * 1e-6, c.scan_ns.load() * 1e-6, c.pack_ns.load() * 1e-6);
    }
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    tr.mark("bookkeeping", nullptr);
    sketch_add_packed_files(s, files.data(), n_paths, n_records, n_short);
    tr.mark("place", nullptr);
  });
}
// ---- files packed once, used many times (fa_packed) ----
int fa_packed_read(const char *const *paths, int32_t n_paths, int protein, fa_packed **out) {
  return guarded([&] {
    FA_REQUIRE(paths && out && n_paths >= 0, FA_ERR_INVALID, "null argument or negative count");
    std::unique_ptr<fa_packed> p(new fa_packed());
    p->protein = protein != 0;
    read_fasta_packed_many(paths, (size_t)n_paths, p->protein, p->files);
    *out = p.release();
  });
}
// more files behind the ones the set holds (read + packed concurrently, like fa_packed_read); all or nothing
int fa_packed_append(fa_packed *p, const char *const *paths, int32_t n_paths) {
  return guarded([&] {
    FA_REQUIRE(p && paths && n_paths >= 0, FA_ERR_INVALID, "null argument or negative count");
    std::vector<PackedFasta> more;
    read_fasta_packed_many(paths, (size_t)n_paths, p->protein, more);
    std::unique_lock<std::shared_mutex> grow(p->mtx);
    p->files.reserve(p->files.size() + more.size());
    for (auto &f : more) p->files.push_back(std::move(f));
  });
}
void fa_packed_free(fa_packed *p) { delete p; }
int fa_packed_info(fa_packed *p, int32_t *n_files, uint64_t *file_bytes, int64_t *records, int64_t *bases) {
  return guarded([&] {
    std::shared_lock<std::shared_mutex> hold(p->mtx);
    if (n_files) *n_files = (int32_t)p->files.size();
    for (size_t i = 0; i < p->files.size(); i++) {
      if (file_bytes) file_bytes[i] = (uint64_t)p->files[i].file_bytes;
      if (records) records[i] = (int64_t)p->files[i].rec_len.size();
      if (bases) { int64_t b = 0; for (int64_t l : p->files[i].rec_len) b += l; bases[i] = b; }
    }
  });
}
int fa_sketch_add_packed(fa_sketch *s, fa_packed *p, int32_t first, int32_t count, int64_t *n_records, int64_t *n_short) {
  return guarded([&] {
    FA_REQUIRE(p, FA_ERR_INVALID, "null packed set");
    std::shared_lock<std::shared_mutex> hold(p->mtx);
    FA_REQUIRE(first >= 0 && count >= 0 && (size_t)first + (size_t)count <= p->files.size(), FA_ERR_INVALID, "file range outside the packed set");
    FA_REQUIRE(p->protein == (s->P.alphabet_size != 4), FA_ERR_INVALID, "the files were packed for the other alphabet");
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    sketch_add_packed_files(s, p->files.data() + first, count, n_records, n_short);
  });
}
int fa_genomes_reload_packed(fa_mapper *m, fa_genomes *g, fa_packed *p, int32_t first, int32_t count) {
  return guarded([&] {
    FA_REQUIRE(g && p, FA_ERR_INVALID, "null argument");
    std::shared_lock<std::shared_mutex> hold(p->mtx);
    FA_REQUIRE(first >= 0 && count >= 0 && (size_t)first + (size_t)count <= p->files.size(), FA_ERR_INVALID, "file range outside the packed set");
    FA_REQUIRE(p->protein == (m->P.alphabet_size != 4), FA_ERR_INVALID, "the files were packed for the other alphabet");
    try { fill_genomes_from_packed(m, g, p->files.data() + first, count, true); } catch (...) { g->reset_empty(); throw; }
  });
}
int fa_sketch_end_genome(fa_sketch *s) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    RefStage add(s->book, OpenGenome::FOLD);
    add.end_genome();
    add.commit(s->book);
  });
}
int fa_sketch_abort_genome(fa_sketch *s) {
  return guarded([&] { std::lock_guard<std::mutex> lock(s->mtx); s->book.cur_total = 0; });
}
int fa_sketch_clear(fa_sketch *s) {
  return guarded([&] { std::lock_guard<std::mutex> lock(s->mtx); s->reset_data(); });
}
int fa_sketch_num_minimizers(fa_sketch *s, int64_t *n) {
  return guarded([&] { std::lock_guard<std::mutex> lock(s->mtx); s->flush(); *n = s->nrec; });
}
int fa_sketch_get_minimizers(fa_sketch *s, uint32_t *hash, int32_t *seq_id, int32_t *wpos) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    s->flush();
    if (s->nrec == 0) return;
    s->rec.store(hash, seq_id, wpos, (size_t)s->nrec, hipMemcpyDeviceToHost, s->stream.get());
    FA_HIP(hipStreamSynchronize(s->stream));
  });
}
int fa_sketch_num_genomes(fa_sketch *s, int64_t *n) {
  return guarded([&] { *n = (int64_t)s->book.lengths.size(); });
}
int fa_sketch_get_state(fa_sketch *s, uint64_t *lengths, int32_t *sbf, int64_t *counter) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    for (size_t i = 0; i < s->book.lengths.size(); i++) { lengths[i] = s->book.lengths[i]; sbf[i] = s->book.seqs_by_file[i]; }
    *counter = s->book.counter;
  });
}
int fa_sketch_set_state(fa_sketch *s, int64_t n_genomes, const uint64_t *lengths, const int32_t *sbf, int64_t counter,
                        int64_t n_min, const uint32_t *hash, const int32_t *seq_id, const int32_t *wpos) {
  return guarded([&] { sketch_set_state(s, n_genomes, lengths, sbf, counter, n_min, hash, seq_id, wpos, hipMemcpyHostToDevice); });
}

// Device-pointer variants of the two calls above: the minimizer records never leave HBM.  Used by the multi-GPU index
// build (every rank sketches a share of the references, the shards are all-gathered over RCCL into
// tensors the caller owns, and every rank loads the merged records).  The caller synchronises its own stream before
// the call; the library synchronises its stream before returning.
int fa_sketch_get_minimizers_device(fa_sketch *s, int64_t cap, uint32_t *d_hash, int32_t *d_seq_id, int32_t *d_wpos) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(s->mtx);
    bind_device(s->device);
    s->flush();
    FA_REQUIRE(cap >= s->nrec, FA_ERR_INVALID, "destination holds fewer records than the sketch");
    if (s->nrec == 0) return;
    s->rec.store(d_hash, d_seq_id, d_wpos, (size_t)s->nrec, hipMemcpyDeviceToDevice, s->stream.get());
    FA_HIP(hipStreamSynchronize(s->stream));
  });
}
int fa_sketch_set_state_device(fa_sketch *s, int64_t n_genomes, const uint64_t *lengths, const int32_t *sbf, int64_t counter,
                               int64_t n_min, const uint32_t *d_hash, const int32_t *d_seq_id, const int32_t *d_wpos) {
  return guarded([&] { sketch_set_state(s, n_genomes, lengths, sbf, counter, n_min, d_hash, d_seq_id, d_wpos, hipMemcpyDeviceToDevice); });
}

// A subset of the genomes as a sketch of its own, and the frequency filter an index of the sketch would have: what maps a
// collection group by group out of one resident sketch (fa_select.hip.h has the semantics and the road).  Both run on the
// sketch's stream and have finished when they return.
int fa_sketch_select(fa_sketch *s, const int32_t *genomes, int32_t n, fa_sketch **out) {
  return guarded([&] {
    sketch_select(s, genomes, n, out);
  });
}

int fa_sketch_frequency(fa_sketch *s, int *threshold, int64_t cap, uint32_t *d_drop_keys, int64_t *n_drop) {
  return guarded([&] {
    sketch_frequency(s, threshold, cap, d_drop_keys, n_drop);
  });
}

int fa_sketch_index(fa_sketch *s, fa_mapper **out) {
  return guarded([&] {
    sketch_index(s, out);
  });
}

void fa_mapper_free(fa_mapper *m) { delete m; }
int fa_mapper_freq_threshold(fa_mapper *m, int *thr) { *thr = m->freq_threshold; return FA_OK; }
int fa_mapper_lookup_size(fa_mapper *m, int64_t *n) { *n = m->U; return FA_OK; }
int fa_mapper_device(fa_mapper *m, int *device) { *device = m->device; return FA_OK; }
int fa_mapper_lookup_export_device(fa_mapper *m, int64_t cap, uint32_t *d_keys, int32_t *d_counts) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    FA_REQUIRE(cap >= m->U, FA_ERR_INVALID, "destination smaller than the lookup index");
    if (m->U == 0) return;
    FA_HIP(hipMemcpyAsync(d_keys, m->uniq_hash.p, (size_t)m->U * sizeof(uint32_t), hipMemcpyDeviceToDevice, m->stream));
    hipLaunchKernelGGL(k_list_lengths, dim3(ceil_div(m->U, 256)), dim3(256), 0, m->stream, m->uniq_off.p, (int64_t)m->U, d_counts);
    FA_HIP(hipGetLastError());
    FA_HIP(hipStreamSynchronize(m->stream));
  });
}
int fa_mapper_set_global_frequency(fa_mapper *m, int threshold, int64_t n_drop, const uint32_t *d_drop_keys) {
  return guarded([&] {
    FA_REQUIRE(threshold >= 0 && n_drop >= 0, FA_ERR_INVALID, "negative threshold or key count");
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    m->freq_threshold = threshold;
    if (n_drop > 0 && m->U > 0) {
      hipLaunchKernelGGL(k_drop_keys, dim3(ceil_div(n_drop, 256)), dim3(256), 0, m->stream, d_drop_keys, n_drop, m->table_bits, m->table.p);
      FA_HIP(hipGetLastError());
    }
    FA_HIP(hipStreamSynchronize(m->stream));
  });
}
int fa_mapper_lookup_keys(fa_mapper *m, uint32_t *keys) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    m->uniq_hash.download(keys, (size_t)m->U, m->stream);
    FA_HIP(hipStreamSynchronize(m->stream));
  });
}
int fa_mapper_lookup_count(fa_mapper *m, uint32_t hash, int64_t *count) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    uint32_t off, cnt;
    *count = host_find(m, hash, &off, &cnt) < 0 ? -1 : (int64_t)cnt;
  });
}
int fa_mapper_lookup_get(fa_mapper *m, uint32_t hash, int32_t *seq_id, int32_t *wpos, int64_t cap) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    uint32_t off, cnt;
    FA_REQUIRE(host_find(m, hash, &off, &cnt) >= 0, FA_ERR_INVALID, "hash not in the lookup index");
    std::vector<uint32_t> ridx(cnt);
    FA_HIP(hipMemcpy(ridx.data(), m->pos_ridx.p + off, (size_t)cnt * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < cnt && (int64_t)i < cap; i++) {
      FA_HIP(hipMemcpy(&seq_id[i], m->rec_seq.p + ridx[i], 4, hipMemcpyDeviceToHost));
      FA_HIP(hipMemcpy(&wpos[i], m->rec_wpos.p + ridx[i], 4, hipMemcpyDeviceToHost));
    }
  });
}
int fa_mapper_num_minimizers(fa_mapper *m, int64_t *n) { *n = m->N; return FA_OK; }
int fa_mapper_get_minimizers(fa_mapper *m, uint32_t *hash, int32_t *seq_id, int32_t *wpos) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    if (m->N == 0) return;
    m->rec_hash.download(hash, (size_t)m->N, m->stream);
    m->rec_seq.download(seq_id, (size_t)m->N, m->stream);
    m->rec_wpos.download(wpos, (size_t)m->N, m->stream);
    FA_HIP(hipStreamSynchronize(m->stream));
  });
}
int fa_mapper_reference_bins(fa_mapper *m, int32_t *bin_length, int64_t *n_contigs, int32_t *contig_bin, int32_t *contig_genome) {
  return guarded([&] {
    FA_REQUIRE(m && bin_length && n_contigs, FA_ERR_INVALID, "null mapper or destination");
    std::lock_guard<std::mutex> lock(m->mtx);
    *bin_length = std::max(m->P.fragment_length - 20, 1);                    // (build_index)
    *n_contigs = m->C;
    if (!contig_bin && !contig_genome) return;
    bind_device(m->device);
    if (contig_bin) m->contig_bin.download(contig_bin, (size_t)m->C + 1, m->stream);
    if (contig_genome) m->contig_genome.download(contig_genome, (size_t)m->C, m->stream);
    FA_HIP(hipStreamSynchronize(m->stream));
  });
}
int fa_mapper_num_genomes(fa_mapper *m, int64_t *n) { *n = (int64_t)m->lengths.size(); return FA_OK; }
int fa_mapper_get_state(fa_mapper *m, uint64_t *lengths, int32_t *sbf) {
  for (size_t i = 0; i < m->lengths.size(); i++) { lengths[i] = m->lengths[i]; sbf[i] = m->seqs_by_file[i]; }
  return FA_OK;
}

int fa_genomes_upload(fa_mapper *m, const void *const *contigs, const int64_t *lengths, const int32_t *contig_genome,
                      int64_t n_contigs, int32_t n_genomes, int char_width, fa_genomes **out) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    auto g = std::make_unique<fa_genomes>();
    fill_genomes(g.get(), m->P, m->stream, contigs, lengths, contig_genome, n_contigs, n_genomes, char_width, nullptr, nullptr, nullptr, false);
    *out = g.release();
  });
}
int fa_genomes_upload_fasta(fa_mapper *m, const char *const *paths, int32_t n_paths, fa_genomes **out) {
  return guarded([&] {
    FA_REQUIRE(n_paths >= 0, FA_ERR_INVALID, "negative count");
    std::unique_ptr<fa_genomes> g(new fa_genomes());
    fill_genomes_from_fasta(m, g.get(), paths, n_paths, false);
    *out = g.release();
  });
}
int fa_genomes_reload_fasta(fa_mapper *m, fa_genomes *g, const char *const *paths, int32_t n_paths) {
  return guarded([&] {
    FA_REQUIRE(g && n_paths >= 0, FA_ERR_INVALID, "null batch or negative count");
    try { fill_genomes_from_fasta(m, g, paths, n_paths, true); } catch (...) { g->reset_empty(); throw; }
  });
}
void fa_genomes_free(fa_genomes *g) { delete g; }
int fa_genomes_info(fa_genomes *g, int32_t *n_genomes, uint64_t *tf, uint64_t *tl, int32_t *ns) {
  if (n_genomes) *n_genomes = g->n_genomes;
  for (int i = 0; i < g->n_genomes; i++) {
    if (tf) tf[i] = g->total_fragments[i];
    if (tl) tl[i] = g->total_length[i];
    if (ns) ns[i] = g->n_short[i];
  }
  return FA_OK;
}
int fa_mapper_query_genomes(fa_mapper *m, fa_genomes *g, int32_t first, int32_t count, fa_cgi_row *rows, int64_t cap,
                            int64_t *n_rows, int rows_device) {
  return guarded([&] {
    WorkspaceLease lease(*m);
    *n_rows = run_query(*m, *lease.w, *g, first, count, rows, cap, rows_device != 0);
  });
}
int fa_mapper_query_genomes_mappings(fa_mapper *m, fa_genomes *g, int32_t first, int32_t count, fa_cgi_row *rows, int64_t cap,
                                     int64_t *n_rows, int rows_device, fa_hit_mapping *maps, int64_t map_cap, int64_t *n_maps,
                                     int maps_device) {
  return guarded([&] {
    WorkspaceLease lease(*m);
    const MapRequest want{maps, map_cap, n_maps, maps_device != 0};
    *n_rows = run_query(*m, *lease.w, *g, first, count, rows, cap, rows_device != 0, &want);
  });
}
int fa_mapper_query_genomes_mappings_stream(fa_mapper *m, fa_genomes *g, int32_t first, int32_t count, fa_cgi_row *rows, int64_t cap,
                                            int64_t *n_rows, int rows_device, fa_mapping_sink sink, void *user, int64_t *n_maps) {
  return guarded([&] {
    WorkspaceLease lease(*m);
    MapRequest want{nullptr, 0, n_maps, false};
    want.stream = true; want.fn = sink; want.user = user;
    *n_rows = run_query(*m, *lease.w, *g, first, count, rows, cap, rows_device != 0, &want);
  });
}
int fa_table_pairs(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes, const uint64_t *query_lengths,
                   const uint64_t *reference_lengths, const fa_table_params *p, fa_pair *pairs, int64_t cap, int64_t *n_pairs,
                   int pairs_device) {
  return guarded([&] {
    table_pairs({rows, n_rows, rows_device != 0, n_genomes, query_lengths, reference_lengths, p}, pairs, cap, n_pairs, pairs_device != 0);
  });
}
int fa_table_clusters(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes, const uint64_t *query_lengths,
                      const uint64_t *reference_lengths, const fa_table_params *p, int32_t *labels, int labels_device,
                      int32_t *n_clusters, int64_t *stats) {
  return guarded([&] {
    table_clusters({rows, n_rows, rows_device != 0, n_genomes, query_lengths, reference_lengths, p},
                   labels, labels_device != 0, n_clusters, stats);
  });
}
int fa_table_representatives(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes, const uint64_t *query_lengths,
                             const uint64_t *reference_lengths, const fa_table_params *p, const int32_t *order, int32_t *labels,
                             double *identity, int out_device, int32_t *n_representatives, int64_t *stats) {
  return guarded([&] {
    table_representatives({rows, n_rows, rows_device != 0, n_genomes, query_lengths, reference_lengths, p},
                          order, labels, identity, out_device != 0, n_representatives, stats);
  });
}
int fa_table_linkage(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes, const uint64_t *query_lengths,
                     const uint64_t *reference_lengths, const fa_table_params *p, float missing, int32_t *labels, int labels_device,
                     int32_t *n_clusters, int64_t *stats) {
  return guarded([&] {
    table_linkage({rows, n_rows, rows_device != 0, n_genomes, query_lengths, reference_lengths, p},
                  missing, labels, labels_device != 0, n_clusters, stats);
  });
}
int fa_table_dendrogram(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes, const uint64_t *query_lengths,
                        const uint64_t *reference_lengths, const fa_table_params *p, float missing, fa_merge *merges, int64_t cap,
                        int64_t *n_merges, int32_t *labels, int out_device, int32_t *n_clusters, int64_t *stats) {
  return guarded([&] {
    table_dendrogram({rows, n_rows, rows_device != 0, n_genomes, query_lengths, reference_lengths, p},
                     missing, merges, cap, n_merges, labels, out_device != 0, n_clusters, stats);
  });
}
int fa_dendrogram_cut(const fa_merge *merges, int64_t n_merges, int merges_device, int32_t n_genomes, const float *min_identity,
                      int32_t n_cuts, int32_t *labels, int labels_device, int32_t *n_clusters) {
  return guarded([&] {
    dendrogram_cut(merges, n_merges, merges_device != 0, n_genomes, min_identity, n_cuts, labels, labels_device != 0, n_clusters);
  });
}
int fa_debug_linkage_order(const int64_t a[4], const int64_t b[4], int *first) {
  return guarded([&] {
    FA_REQUIRE(a && b && first, FA_ERR_INVALID, "null candidate or destination");
    FA_REQUIRE(a[0] >= 0 && b[0] >= 0 && a[1] >= 1 && b[1] >= 1, FA_ERR_INVALID, "a candidate has S >= 0 and |A||B| >= 1");
    FA_REQUIRE(a[2] >= 0 && a[2] <= INT32_MAX && a[3] >= 0 && a[3] <= INT32_MAX && b[2] >= 0 && b[2] <= INT32_MAX && b[3] >= 0 &&
                   b[3] <= INT32_MAX, FA_ERR_INVALID, "a label is a genome number");
    const LinkCand x{a[0], a[1], (int32_t)a[2], (int32_t)a[3]}, y{b[0], b[1], (int32_t)b[2], (int32_t)b[3]};
    *first = link_order(x, y);
  });
}
int fa_table_medoids(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes, const uint64_t *query_lengths,
                     const uint64_t *reference_lengths, const fa_table_params *p, float missing, const int32_t *labels, int32_t n_sets,
                     const double *bonus, int32_t *medoids, double *identity, int64_t *sums, int32_t *sizes, int io_device,
                     int32_t *n_clusters, int64_t *stats) {
  return guarded([&] {
    table_medoids({rows, n_rows, rows_device != 0, n_genomes, query_lengths, reference_lengths, p},
                  missing, labels, n_sets, bonus, medoids, identity, sums, sizes, io_device != 0, n_clusters, stats);
  });
}
int fa_debug_medoid_better(double bonus_b, int64_t s_b, int32_t b, double bonus_a, int64_t s_a, int32_t a, int32_t m, int64_t t[2],
                           int *better) {
  return guarded([&] {
    FA_REQUIRE(t && better, FA_ERR_INVALID, "null destination");
    FA_REQUIRE(medoid_bonus_ok(bonus_a) && medoid_bonus_ok(bonus_b), FA_ERR_INVALID, "a bonus must be a number in [-32768, 32768]");
    FA_REQUIRE(m >= 1 && m <= LINK_MAX_GENOMES && a >= 0 && b >= 0, FA_ERR_INVALID, "a cluster has 1 .. 2^18 members with numbers >= 0");
    FA_REQUIRE(s_a >= 0 && s_b >= 0 && s_a < (1LL << 46) && s_b < (1LL << 46), FA_ERR_INVALID, "a centrality sum lies in [0, 2^46)");
    t[0] = medoid_t(s_b, medoid_qb(bonus_b), m);
    t[1] = medoid_t(s_a, medoid_qb(bonus_a), m);
    *better = medoid_better(t[0], b, t[1], a) ? 1 : 0;
  });
}
int fa_mappings_profile(const fa_hit_mapping *maps, int64_t n_maps, int maps_device, int32_t n_queries, const int64_t *fragment_offsets,
                        int32_t n_references, const int32_t *query_labels, const int32_t *reference_labels, const int32_t *self_reference,
                        float min_identity, int32_t *d_count, int64_t *d_sum, float *d_lowest, int64_t *stats) {
  return guarded([&] {
    mappings_profile(maps, n_maps, maps_device != 0, n_queries, fragment_offsets, n_references, query_labels, reference_labels, self_reference,
                     min_identity, d_count, d_sum, d_lowest, stats);
  });
}
int fa_profile_summary(const int32_t *d_count, const int64_t *d_sum, int32_t n_queries, const int64_t *fragment_offsets,
                       const int32_t *min_count, int32_t n_sets, int64_t *fragments, int64_t *hits, int64_t *sum, int out_device) {
  return guarded([&] {
    profile_summary(d_count, d_sum, n_queries, fragment_offsets, min_count, n_sets, fragments, hits, sum, out_device != 0);
  });
}
int fa_profile_chunk(int32_t *records_per_workgroup, int32_t *lds_fragments) {
  return guarded([&] {
    FA_REQUIRE(records_per_workgroup && lds_fragments, FA_ERR_INVALID, "null destination");
    *records_per_workgroup = PROF_CHUNK;
    *lds_fragments = PROF_LDS_FRAGMENTS;
  });
}
int fa_debug_profile_road(int32_t road) {
  return guarded([&] {
    FA_REQUIRE(road >= 0 && road <= 2, FA_ERR_INVALID, "road 0 (the policy), 1 (global atomics) or 2 (on chip wherever it fits)");
    g_profile_road.store(road);
  });
}
int fa_mappings_reference_profile(const fa_hit_mapping *maps, int64_t n_maps, int maps_device, int32_t n_queries, int32_t n_references,
                                  int32_t n_contigs, const int32_t *contig_bin, const int32_t *contig_genome, int32_t bin_length,
                                  const int32_t *query_labels, const int32_t *reference_labels, const int32_t *self_reference,
                                  float min_identity, int32_t *d_count, int64_t *d_sum, float *d_lowest, int64_t *stats) {
  return guarded([&] {
    mappings_reference_profile(maps, n_maps, maps_device != 0, n_queries, n_references, n_contigs, contig_bin, contig_genome, bin_length,
                               query_labels, reference_labels, self_reference, min_identity, d_count, d_sum, d_lowest, stats);
  });
}
int fa_reference_profile_chunk(int32_t *records_per_workgroup) {
  return guarded([&] {
    FA_REQUIRE(records_per_workgroup, FA_ERR_INVALID, "null destination");
    *records_per_workgroup = REFPROF_CHUNK;
  });
}
int fa_profile_regions(const int32_t *d_count, const int64_t *d_sum, int32_t n_segments, const int64_t *segment_offsets,
                       const int32_t *need, int below, int32_t min_length, fa_profile_region *regions, int64_t cap,
                       int64_t *n_regions, int out_device) {
  return guarded([&] {
    profile_regions(d_count, d_sum, n_segments, segment_offsets, need, below != 0, min_length, regions, cap, n_regions, out_device != 0);
  });
}
int fa_profile_regions_chunk(int32_t *entries_per_workgroup) {
  return guarded([&] {
    FA_REQUIRE(entries_per_workgroup, FA_ERR_INVALID, "null destination");
    *entries_per_workgroup = REG_CHUNK;
  });
}
int fa_table_best(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_queries, int32_t n_references,
                  const uint64_t *query_lengths, const uint64_t *reference_lengths, const fa_best_params *p, fa_cgi_row *best,
                  int64_t *offsets, int64_t cap, int64_t *n_best, int out_device, int64_t *stats) {
  return guarded([&] {
    table_best(rows, n_rows, rows_device != 0, n_queries, n_references, query_lengths, reference_lengths, p, best, offsets, cap, n_best,
               out_device != 0, stats);
  });
}
int fa_screen_tile(int32_t s, int32_t *tile) {
  return guarded([&] {
    FA_REQUIRE(tile && s >= 1 && s <= SCR_MAX_S, FA_ERR_INVALID, "the signature size must be in [1, 4096]");
    *tile = screen_tile(s);
  });
}
int fa_screen_signatures(const uint32_t *d_hash, const int32_t *d_seq_id, int64_t n_records, const int32_t *sbf, int32_t n_genomes,
                         int32_t s, uint32_t *d_sig, int32_t *d_count) {
  return guarded([&] { screen_signatures(d_hash, d_seq_id, n_records, sbf, n_genomes, s, d_sig, d_count); });
}
int fa_genomes_signatures(fa_mapper *m, fa_genomes *g, int32_t first, int32_t count, int32_t s, int64_t pass_fragments, uint32_t *d_sig,
                          int32_t *d_count, int64_t *stats) {
  return guarded([&] { genomes_signatures(m, g, first, count, s, pass_fragments, d_sig, d_count, stats); });
}
int fa_screen_pairs(const uint32_t *d_sig_a, const int32_t *d_count_a, int32_t n_a, const uint32_t *d_sig_b, const int32_t *d_count_b,
                    int32_t n_b, int32_t s, int triangular, int32_t jn, int32_t jd, fa_screen_pair *pairs, int64_t cap, int64_t *n_pairs,
                    int pairs_device, int64_t *stats) {
  return guarded([&] {
    screen_pairs(d_sig_a, d_count_a, n_a, d_sig_b, d_count_b, n_b, s, triangular != 0, jn, jd, pairs, cap, n_pairs, pairs_device != 0, stats);
  });
}
int fa_screen_groups(const fa_screen_pair *pairs, int64_t n_pairs, int pairs_device, int32_t n_genomes, int32_t *labels, int labels_device,
                     int32_t *n_groups) {
  return guarded([&] { screen_groups(pairs, n_pairs, pairs_device != 0, n_genomes, labels, labels_device != 0, n_groups); });
}
int fa_screen_contents(const uint32_t *d_hash, const int32_t *d_seq_id, int64_t n_records, const int32_t *sbf, int32_t n_genomes,
                       uint32_t *d_ent_hash, int32_t *d_ent_genome, int64_t cap, int64_t *n_entries) {
  return guarded([&] { screen_contents(d_hash, d_seq_id, n_records, sbf, n_genomes, d_ent_hash, d_ent_genome, cap, n_entries); });
}
int fa_screen_contain_slice(int32_t *slice) {
  return guarded([&] {
    FA_REQUIRE(slice, FA_ERR_INVALID, "null destination");
    *slice = CNT_SLICE;
  });
}
int fa_screen_contained(const uint32_t *d_sig, const int32_t *d_count, int32_t n_a, int32_t s, const uint32_t *d_ent_hash,
                        const int32_t *d_ent_genome, int64_t n_entries, int32_t n_b, int32_t cn, int32_t cd, fa_screen_pair *pairs,
                        int64_t cap, int64_t *n_pairs, int pairs_device, int64_t *stats) {
  return guarded([&] {
    screen_contained(d_sig, d_count, n_a, s, d_ent_hash, d_ent_genome, n_entries, n_b, false, nullptr, cn, cd, pairs, cap, n_pairs,
                     pairs_device != 0, stats);
  });
}
int fa_screen_contained_winner(const uint32_t *d_sig, const int32_t *d_count, int32_t n_a, int32_t s, const uint32_t *d_ent_hash,
                               const int32_t *d_ent_genome, int64_t n_entries, int32_t n_b, const int32_t *d_weight, int32_t cn, int32_t cd,
                               fa_screen_pair *pairs, int64_t cap, int64_t *n_pairs, int pairs_device, int64_t *stats) {
  return guarded([&] {
    screen_contained(d_sig, d_count, n_a, s, d_ent_hash, d_ent_genome, n_entries, n_b, true, d_weight, cn, cd, pairs, cap, n_pairs,
                     pairs_device != 0, stats);
  });
}
int fa_debug_contain_winner_threads(int32_t threads) {
  return guarded([&] {
    FA_REQUIRE(threads == 0 || threads == 512 || threads == 1024, FA_ERR_INVALID, "512 or 1024 threads, or 0 for the default");
    g_winner_threads.store(threads ? threads : WIN_THREADS);
  });
}
int fa_mapper_set_mapping_stage(fa_mapper *m, int64_t records) {
  return guarded([&] {
    FA_REQUIRE(m && records >= 1, FA_ERR_INVALID, "the mapping stage holds at least one record");
    std::lock_guard<std::mutex> lock(m->mtx);
    m->map_stage = records;
  });
}
int fa_rules_default(fa_rules *out) {
  return guarded([&] { FA_REQUIRE(out, FA_ERR_INVALID, "null destination"); *out = default_rules(); });
}
static void validate_rules(const fa_rules &r) {
  FA_REQUIRE(r.l2_confidence > 0.0f && r.l2_confidence < 1.0f, FA_ERR_INVALID, "l2_confidence must lie strictly inside (0, 1)");
  FA_REQUIRE(r.slide_end == 0 || r.slide_end == 1, FA_ERR_INVALID, "slide_end must be 0 (windows) or 1 (fragment)");
  FA_REQUIRE(r.cgi_ties == 0 || r.cgi_ties == 1, FA_ERR_INVALID, "cgi_ties must be 0 (smallest) or 1 (largest)");
}
// The interval only feeds the pass table (StatTables::pass_shared): it is rebuilt and uploaded, and the table it replaces is
// retired like the generations ensure_luts outgrows -- calls in flight read it to their end.  The other two rules are argument
// words of the kernels of the calls that start from now on.
int fa_mapper_set_rules(fa_mapper *m, const fa_rules *r) {
  return guarded([&] {
    FA_REQUIRE(r, FA_ERR_INVALID, "null rules");
    validate_rules(*r);
    FA_REQUIRE(m, FA_ERR_INVALID, "null mapper");
    std::lock_guard<std::mutex> lock(m->mtx);
    if (same_rules(m->rules, *r)) return;
    if (r->l2_confidence != m->stats.ci) {
      StatTables next = m->stats;                            // (a failed upload leaves the mapper as it was)
      next.set_ci(r->l2_confidence);
      require_no_zero_pass(next);                           // (refused: the mapper keeps its rules)
      if (m->d_pass.p) {
        bind_device(m->device);
        DevBuf<int32_t> d_next;
        d_next.upload(next.pass_shared, m->stream);
        FA_HIP(hipStreamSynchronize(m->stream));
        m->retired_i32.push_back(std::move(m->d_pass));
        m->d_pass = std::move(d_next);
      }
      m->stats = std::move(next);
    }
    m->rules = *r;
  });
}
int fa_mapper_get_rules(fa_mapper *m, fa_rules *out) {
  return guarded([&] {
    FA_REQUIRE(m && out, FA_ERR_INVALID, "null mapper or destination");
    std::lock_guard<std::mutex> lock(m->mtx);
    *out = m->rules;
  });
}
int fa_pass_threshold(int sketch_size, int k, float identity, float ci, int *min_shared) {
  return guarded([&] {
    FA_REQUIRE(min_shared && sketch_size > 0 && k >= 1, FA_ERR_INVALID, "sketch_size and k must be positive");
    FA_REQUIRE(ci > 0.0f && ci < 1.0f, FA_ERR_INVALID, "the confidence interval must lie strictly inside (0, 1)");
    FA_REQUIRE(!stat_zero_passes_alone(sketch_size, k, identity, ci), FA_ERR_UNSUPPORTED,
               "a mapping of no shared record passes alone: no threshold states this filter (a mapper refuses these parameters)");
    *min_shared = stat_pass_threshold(sketch_size, k, identity, ci);
  });
}
int fa_mapper_mapping_memory(fa_mapper *m, int64_t out[4]) {
  return guarded([&] {
    FA_REQUIRE(m && out, FA_ERR_INVALID, "null mapper or destination");
    std::lock_guard<std::mutex> lock(m->mtx);
    for (int i = 0; i < 4; i++) out[i] = 0;
    if (m->last_map_ws < 0) return;
    const Workspace &w = m->ws[m->last_map_ws];
    out[0] = w.map_stage.records;
    out[1] = out[2] = (int64_t)w.map_stage.bytes();
    out[3] = (int64_t)w.winners.block;
  });
}
static int query_one(fa_mapper *m, const void *const *contigs, const int64_t *lengths, int n_contigs, int char_width,
                     fa_cgi_row *rows, int64_t cap, int64_t *n_rows, int *n_short, uint64_t *total_fragments,
                     uint64_t *total_length, const MapRequest *want) {
  return guarded([&] { query_one_call(m, contigs, lengths, n_contigs, char_width, rows, cap, n_rows, n_short, total_fragments, total_length, want); });
}
int fa_mapper_query(fa_mapper *m, const void *const *contigs, const int64_t *lengths, int n_contigs, int char_width,
                    fa_cgi_row *rows, int64_t cap, int64_t *n_rows, int *n_short, uint64_t *total_fragments,
                    uint64_t *total_length) {
  return query_one(m, contigs, lengths, n_contigs, char_width, rows, cap, n_rows, n_short, total_fragments, total_length, nullptr);
}
int fa_mapper_query_mappings(fa_mapper *m, const void *const *contigs, const int64_t *lengths, int n_contigs, int char_width,
                             fa_cgi_row *rows, int64_t cap, int64_t *n_rows, int *n_short, uint64_t *total_fragments,
                             uint64_t *total_length, fa_hit_mapping *maps, int64_t map_cap, int64_t *n_maps) {
  const MapRequest want{maps, map_cap, n_maps, false};
  return query_one(m, contigs, lengths, n_contigs, char_width, rows, cap, n_rows, n_short, total_fragments, total_length, &want);
}
int fa_mapper_query_mappings_stream(fa_mapper *m, const void *const *contigs, const int64_t *lengths, int n_contigs, int char_width,
                                    fa_cgi_row *rows, int64_t cap, int64_t *n_rows, int *n_short, uint64_t *total_fragments,
                                    uint64_t *total_length, fa_mapping_sink sink, void *user, int64_t *n_maps) {
  MapRequest want{nullptr, 0, n_maps, false};
  want.stream = true; want.fn = sink; want.user = user;
  return query_one(m, contigs, lengths, n_contigs, char_width, rows, cap, n_rows, n_short, total_fragments, total_length, &want);
}

int fa_mapper_debug_mappings(fa_mapper *m, fa_mapping *out, int64_t cap, int64_t *n) {
  return guarded([&] {
    LastPass last(m);
    Workspace &w = last.w;
    ensure_luts(*m, 1);
    int64_t k = 0;
    if (last.held) {
      const uint32_t L = w.last_loci;
      std::vector<int32_t> lf(L), ls(L), lp(L), lsh(L), qs((size_t)w.last_F);
      w.q_size.download(qs.data(), (size_t)w.last_F, w.stream);
      last.copy({{lf.data(), w.l_frag.p}, {ls.data(), w.l_seq.p}, {lp.data(), w.l_pos.p}, {lsh.data(), w.l_shared.p}}, L);
      // (the filter of doL2Mapping at the interval the call ran with, which the mapper may have left since)
      std::vector<int32_t> own;
      if (w.rules.l2_confidence != m->stats.ci) own = m->stats.pass_shared_at(w.rules.l2_confidence);
      const std::vector<int32_t> &pass_shared = own.empty() ? m->stats.pass_shared : own;
      for (uint32_t i = 0; i < L; i++) {
        int s = qs[lf[i]];
        if (lsh[i] < pass_shared[s]) continue;
        if (k < cap) {
          fa_mapping r;
          r.query_seq_id = lf[i]; r.ref_seq_id = ls[i]; r.ref_start_pos = lp[i]; r.sketch_size = s;
          r.conserved = lsh[i]; r.query_id = 0;
          out[k] = r;
        }
        k++;
      }
    }
    *n = k;
  });
}
int fa_mapper_debug_l1(fa_mapper *m, int32_t *frag, int32_t *seq_id, int32_t *rs, int32_t *re, int64_t cap, int64_t *n) {
  return guarded([&] {
    LastPass last(m);
    const Workspace &w = last.w;
    *n = last.copy({{frag, w.l_frag.p}, {seq_id, w.l_seq.p}, {rs, w.l_start.p}, {re, w.l_end.p}}, cap);
  });
}
int fa_mapper_debug_query_sketch(fa_mapper *m, int64_t fragment, uint32_t *hashes, int32_t cap, int32_t *sketch_size) {
  return guarded([&] {
    LastPass last(m);
    const Workspace &w = last.w;
    if (!last.held || fragment < 0 || fragment >= w.last_F) throw Error(FA_ERR_INVALID, "fragment out of range");
    int32_t s = 0;
    FA_HIP(hipMemcpy(&s, w.q_size.p + fragment, 4, hipMemcpyDeviceToHost));
    *sketch_size = s;
    int c = std::min(s, cap);
    if (c > 0) FA_HIP(hipMemcpy(hashes, w.q_hash.p + (size_t)fragment * m->qcap, (size_t)c * 4, hipMemcpyDeviceToHost));
  });
}
int fa_debug_sketch_sequence(const fa_params *params, const void *data, int64_t length, int char_width, uint32_t *hash,
                             int32_t *wpos, int64_t cap, int64_t *n) {
  return guarded([&] {
    validate_params(*params);
    debug_sketch_sequence(params, data, length, char_width, hash, wpos, cap, n);
  });
}

// development probe: how many 128-thread workgroups with `lds_bytes` of dynamic LDS does the chip hold at once, right now?
__global__ void k_probe_occupancy(unsigned *alive, unsigned *peak, int spin) {
  extern __shared__ unsigned char probe_lds[];
  if (threadIdx.x == 0) { unsigned a = atomicAdd(alive, 1u) + 1u; atomicMax(peak, a); }
  probe_lds[threadIdx.x] = (unsigned char)threadIdx.x;
  __syncthreads();
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  while (__builtin_amdgcn_s_memtime() - t0 < (unsigned long long)spin) __builtin_amdgcn_s_sleep(8);
  __syncthreads();
  if (threadIdx.x == 0) atomicSub(alive, 1u);
  if (probe_lds[(threadIdx.x + 1) & 63] == 255 && spin < 0) alive[1] = 1;
}
int fa_debug_probe_occupancy(int lds_bytes, int *peak_alive) {
  return guarded([&] {
    require_device();
    DevBuf<unsigned> d;
    d.ensure(16);
    FA_HIP(hipMemset(d.p, 0, 64));
    hipLaunchKernelGGL(k_probe_occupancy, dim3(4096), dim3(128), (size_t)lds_bytes, 0, d.p, d.p + 4, 200000);
    FA_HIP(hipDeviceSynchronize());
    unsigned h[8];
    FA_HIP(hipMemcpy(h, d.p, 32, hipMemcpyDeviceToHost));
    *peak_alive = (int)h[4];
  });
}
int fa_mapper_debug_items(fa_mapper *m, void *out, int64_t bytes) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    Workspace &w = m->ws[m->last_ws];
    FA_REQUIRE(bytes >= 0 && (size_t)bytes <= w.items.cap, FA_ERR_INVALID, "more bytes than the event arena holds");
    FA_HIP(hipMemcpy(out, w.items.p, (size_t)bytes, hipMemcpyDeviceToHost));
  });
}
int fa_mapper_debug_links(fa_mapper *m, int32_t *prev, int32_t *fwd, int32_t *bwd, uint8_t *flags, int64_t cap, int64_t *n) {
  return guarded([&] {
    std::lock_guard<std::mutex> lock(m->mtx);
    bind_device(m->device);
    const size_t c = (size_t)std::max<int64_t>(0, std::min<int64_t>(m->N, cap));
    if (c) {
      FA_HIP(hipMemcpy(prev, m->rec_prev.p, c * 4, hipMemcpyDeviceToHost));
      FA_HIP(hipMemcpy(fwd, m->rec_fwd.p, c * 4, hipMemcpyDeviceToHost));
      FA_HIP(hipMemcpy(bwd, m->rec_bwd.p, c * 4, hipMemcpyDeviceToHost));
      FA_HIP(hipMemcpy(flags, m->rec_flags.p, c, hipMemcpyDeviceToHost));
    }
    *n = m->N;
  });
}
int fa_mapper_debug_locus_events(fa_mapper *m, uint32_t *events, int64_t cap, int64_t *n) {
  return guarded([&] {
    LastPass last(m);
    *n = last.copy({{events, last.w.l_nev.p}}, cap);
  });
}
int fa_mapper_set_stage_events(fa_mapper *m, int on) {
  std::lock_guard<std::mutex> lock(m->mtx);
  m->stage_events = on != 0;
  return FA_OK;
}
int fa_mapper_last_timings(fa_mapper *m, float *ms, int n) {
  std::lock_guard<std::mutex> lock(m->mtx);
  for (int i = 0; i < n && i < MS_SLOTS; i++) ms[i] = m->ws[m->last_ws].last_ms[i];
  return FA_OK;
}
int fa_mapper_debug_spec(fa_mapper *m, int64_t *out, int n) {
  std::lock_guard<std::mutex> lock(m->mtx);
  const Spec &s = m->spec;
  const Forms &f = m->ws[m->last_ws].last_forms;
  auto ppm = [](float share) { return (int64_t)std::lround((double)share * 1e6); };
#define FA_SPEC_VALUE(name, expr) expr,
  const int64_t v[] = {FA_SPEC_FIELDS(FA_SPEC_VALUE)};
#undef FA_SPEC_VALUE
  for (int i = 0; i < n; i++) out[i] = i < (int)(sizeof(v) / sizeof(v[0])) ? v[i] : 0;
  return FA_OK;
}
int fa_mapper_stream(fa_mapper *m, void **stream) { *stream = (void *)m->stream; return FA_OK; }

int fa_bench_sketch_kernel(fa_mapper *m, fa_genomes *g, int repeat, float *ms_per_launch, uint64_t *bases, uint64_t *minimizers) {
  return guarded([&] {
    bench_sketch_kernel(m, g, repeat, ms_per_launch, bases, minimizers);
  });
}


}  // extern "C"
