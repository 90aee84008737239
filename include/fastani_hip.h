/* include/fastani_hip.h
 *
 * C ABI of libfastani_hip.so: the MI355X-native FastANI fragment-mapping
 * engine that stands in for the C++ symbols pyfastani's Cython module
 * cimports (there is no plugin registry in the reference; the boundary IS
 * that cimport surface).  Every entry point names the reference
 * interface it replaces (paths relative to the pyfastani checkout).
 *
 * Conventions
 *   - plain pointers and sizes only; opaque handles own all device memory;
 *   - every function returns 0 on success, non-zero on failure; the message
 *     is available from fa_last_error() (thread-local); nothing throws
 *     across the boundary (reference: `except +` / `except 1 nogil`,
 *     include/fastani/map/compute_map.pxd:31-36, src/pyfastani/_fastani.pyx:164,893);
 *   - input buffers are borrowed for the duration of the call
 *     (_fastani.pyx:1095 memoryview over caller memory);
 *   - contigs are passed as (pointer, length, char_width) with char_width
 *     1, 2 or 4 = the PyUnicode kind (_fastani.pyx:633-645,1073-1092);
 *   - there is NO CPU fallback: without a HIP device the compute entry points
 *     fail with FA_ERR_NO_DEVICE.
 */
#ifndef FASTANI_HIP_H
#define FASTANI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_OK 0
#define FA_ERR_INVALID 1     /* bad argument (maps to ValueError)              */
#define FA_ERR_NO_DEVICE 2   /* no HIP device / HIP runtime error (RuntimeError) */
#define FA_ERR_NOMEM 3       /* host or device allocation failed (MemoryError)  */
#define FA_ERR_UNSUPPORTED 4 /* parameter regime outside the HIP path           */
#define FA_ERR_INTERNAL 5
#define FA_ERR_IO 6          /* file could not be opened / mapped (OSError)      */
#define FA_ERR_BUFFER 7      /* FASTA header longer than the reference's line buffer (BufferError) */

typedef struct fa_sketch fa_sketch;   /* skch::Sketch under construction + pyfastani bookkeeping */
typedef struct fa_mapper fa_mapper;   /* indexed reference, resident in HBM (skch::Sketch after index() + skch::Map) */
typedef struct fa_genomes fa_genomes; /* a batch of query genomes packed 2-bit and resident in HBM */

/* skch::Parameters, include/fastani/map/map_parameters.pxd:9-24 (fields the path reads) */
typedef struct fa_params {
  int32_t kmer_size;            /* kmerSize            */
  int32_t window_size;          /* windowSize          */
  int32_t fragment_length;      /* minReadLength       */
  int32_t alphabet_size;        /* alphabetSize: 4 nucleotide, 20 protein */
  float min_fraction;           /* minFraction         */
  float percentage_identity;    /* percentageIdentity  */
  double p_value;               /* p_value             */
  uint64_t reference_size;      /* referenceSize       */
} fa_params;

/* cgi::CGI_Results, include/fastani/cgi/cgid_types.pxd:19-27, plus the query index of a batch */
typedef struct fa_cgi_row {
  int32_t query_id;               /* position of the query genome in the batch (qryGenomeId) */
  int32_t ref_genome_id;          /* refGenomeId          */
  int32_t count_seq;              /* countSeq  -> Hit.matches   */
  int32_t total_query_fragments;  /* totalQueryFragments -> Hit.fragments */
  float identity;                 /* identity  -> Hit.identity  */
} fa_cgi_row;

/* one L2 mapping, include/fastani/map/base_types.pxd:52-63 (fields consumed downstream) */
typedef struct fa_mapping {
  int32_t query_seq_id;     /* querySeqId: fragment number inside its query genome */
  int32_t ref_seq_id;       /* refSeqId   */
  int32_t ref_start_pos;    /* refStartPos (= meanOptimalPos) */
  int32_t sketch_size;      /* sketchSize */
  int32_t conserved;        /* conservedSketches */
  int32_t query_id;
} fa_mapping;

/* one mapping that computeCGI kept: best of its query fragment for this reference genome (step 1) and best of its
 * reference bin (step 2); the rows' count_seq of a pair = its number of records, the rows' identity = the float32
 * mean of their identities in the order given.  What FastANI's --visualize dumps per fragment (Parameters.visualize,
 * include/fastani/map/map_parameters.pxd:22-24). */
typedef struct fa_hit_mapping {
  int32_t query_id;         /* position of the query genome in the batch, as in fa_cgi_row */
  int32_t query_seq_id;     /* querySeqId: fragment number inside its query genome */
  int32_t ref_genome_id;    /* refGenomeId */
  int32_t ref_seq_id;       /* refSeqId: contig of the reference */
  int32_t ref_start_pos;    /* refStartPos (= meanOptimalPos) on that contig */
  int32_t sketch_size;      /* sketchSize of the query fragment */
  int32_t conserved;        /* conservedSketches */
  float identity;           /* nucIdentity, the value the row averages */
} fa_hit_mapping;           /* 32 bytes */

/* The readings of FastANI's arithmetic that the reference's sources leave open and that move results:
 * a setting of the mapper, not of the index -- one index can be queried under several.  fa_rules_default gives the values
 * every mapper starts with. */
typedef struct fa_rules {
  float   l2_confidence;   /* 0.9f  | any value strictly inside (0, 1): the doL2Mapping site only */
  int32_t slide_end;       /* 0 = rangeEndPos + countMinimizerWindows | 1 = rangeEndPos + fragment_length */
  int32_t cgi_ties;        /* 0 = smallest (refSeqId, refStartPos) / querySeqId | 1 = largest */
} fa_rules;

/* ---- library ---------------------------------------------------------- */
const char *fa_last_error(void);
int fa_version(void);
/* Device memory the library's handles give back is kept in a per-device pool and reused (on this runtime memory that went
 * through hipFree is scrubbed before it is handed out again, which made the second index build of a process twelve times
 * slower than the first).  fa_device_trim returns everything the pool holds to the runtime (*held_bytes, if not NULL: what
 * it held); FA_POOL_MAX_GB (default 96, 0 = no pool) bounds it. */
int fa_device_trim(uint64_t *held_bytes);
int fa_device_count(int *count);
int fa_set_device(int device);            /* one process per GPU: call once per rank */

/* ---- parameter statistics (host) -------------------------------------- */
/* skch::Stat::recommendedWindowSize, include/fastani/map/map_stats.pxd:22-29, called _fastani.pyx:553-560.
 * *window = -1 when no sketch size reaches the p-value cut-off (upstream reads an uninitialised value there). */
int fa_recommended_window_size(double p_value, int k, int alphabet_size, float identity, int fragment_length,
                               uint64_t reference_size, int *window);
/* skch::Stat::estimateMinimumHitsRelaxed, map_stats.pxd:11, called _fastani.pyx:951 */
int fa_estimate_minimum_hits_relaxed(int sketch_size, int k, float identity, int *hits);
/* nucIdentity / nucIdentityUpperBound of skch::Map::doL2Mapping for (shared, sketch_size) */
int fa_mapping_identity(int shared, int sketch_size, int k, float *identity, float *upper_bound);
/* host, no device: smallest shared count of a sketch of size s whose upper-bound identity passes, at interval ci
 * (the filter of skch::Map::doL2Mapping; sketch_size + 1 when no count passes).  FA_ERR_UNSUPPORTED where a mapping of NO
 * shared record passes while one of a single shared record does not (k <= 7, sketches of hundreds of records, identities below
 * ~18 %): no threshold states that filter, and a mapper refuses a query or fa_mapper_set_rules under such parameters */
int fa_pass_threshold(int sketch_size, int k, float identity, float ci, int *min_shared);
/* skch::CommonFunc::getHash, include/fastani/map/common_func.pxd:12 (host twin of the device function) */
uint32_t fa_hash(const void *kmer, int length);

/* ---- Sketch: reference side ------------------------------------------- */
/* `new Sketch_t(param)`, _fastani.pyx:476 */
int fa_sketch_new(const fa_params *params, fa_sketch **out);
void fa_sketch_free(fa_sketch *s);
/* one iteration of the contig loop of Sketch._add_draft, _fastani.pyx:629-683 (addMinimizers on device, lazily).
 * *added = 0 when the contig is shorter than the window or k-mer size (the UserWarning case, :670-677). */
int fa_sketch_add_contig(fa_sketch *s, const void *data, int64_t length, int char_width, int *added);
/* tail of Sketch._add_draft, _fastani.pyx:686-690: closes the genome, records its fragment-rounded length */
int fa_sketch_end_genome(fa_sketch *s);
/* the exception path of Sketch._add_draft: the reference sums the genome length in a local (`total`, _fastani.pyx:618,680)
 * that is lost when a contig raises half-way, while the contigs already added stay in the sketch; call this from the
 * binding's exception handler so that the abandoned genome's length is not carried into the next one. */
int fa_sketch_abort_genome(fa_sketch *s);
/* Sketch.clear, _fastani.pyx:746-767 */
int fa_sketch_clear(fa_sketch *s);
/* len(Sketch.minimizers) / Minimizers.__getitem__, _fastani.pyx:1222-1235 (device -> host read-back) */
int fa_sketch_num_minimizers(fa_sketch *s, int64_t *n);
int fa_sketch_get_minimizers(fa_sketch *s, uint32_t *hash, int32_t *seq_id, int32_t *wpos);
/* Sketch.__getstate__/__setstate__, _fastani.pyx:572-591 */
int fa_sketch_num_genomes(fa_sketch *s, int64_t *n);
int fa_sketch_get_state(fa_sketch *s, uint64_t *lengths, int32_t *sequences_by_file, int64_t *counter);
int fa_sketch_set_state(fa_sketch *s, int64_t n_genomes, const uint64_t *lengths, const int32_t *sequences_by_file,
                        int64_t counter, int64_t n_minimizers, const uint32_t *hash, const int32_t *seq_id,
                        const int32_t *wpos);
/* Device-pointer variants of fa_sketch_get_minimizers / fa_sketch_set_state (same record layout as the pickled state,
 * _fastani.pyx:572-591): the three arrays live in HBM buffers owned by the caller (e.g. torch tensors), so the
 * multi-GPU index build can all-gather minimizer shards over RCCL without a host round trip.
 * `cap` is the capacity of the destination arrays in records. */
int fa_sketch_get_minimizers_device(fa_sketch *s, int64_t cap, uint32_t *d_hash, int32_t *d_seq_id, int32_t *d_wpos);
int fa_sketch_set_state_device(fa_sketch *s, int64_t n_genomes, const uint64_t *lengths, const int32_t *sequences_by_file,
                               int64_t counter, int64_t n_minimizers, const uint32_t *d_hash, const int32_t *d_seq_id,
                               const int32_t *d_wpos);
/* Sketch.index, _fastani.pyx:769-806: Sketch_t::index() + computeFreqHist(); ownership of the data moves to the
 * mapper and the sketch is left cleared but usable. */
int fa_sketch_index(fa_sketch *s, fa_mapper **out);

/* ---- a collection mapped group by group out of one resident sketch ---- */
/* What comes between the screen and a mapper when a collection is larger than one index: a Sketch holds 12 bytes per record
 * and an index is bound to 2^31 of them, so a collection sketched once is cut into its groups here, each group indexed and
 * mapped on its own, and the frequency filter of the WHOLE collection installed in every group's mapper
 * (fa_mapper_set_global_frequency) -- the group's rows are then the rows the one big index would give for its references.
 * No reference counterpart.  With sbf = sequencesByFileInfo of s, first(g) = g ? sbf[g-1] : 0, c(g) = sbf[g] - first(g):
 *   1. Selection.  genomes[0..n) is a HOST array, strictly ascending, every entry in [0, n_genomes).  *out is a new sketch
 *      with the fa_params of s, on its device, that holds those genomes:  lengths'[i] = lengths[genomes[i]],
 *      sbf'[i] = sum over j <= i of c(genomes[j]),  counter' = sbf'[n-1] (0 for n == 0).
 *   2. Records.  The records of genome g are those with contig id in [first(g), sbf[g]): a contiguous range, records being
 *      sorted by contig id.  The records of genomes[i] are copied in their order with hash and window position unchanged;
 *      their contig id becomes  seq_id - first(genomes[i]) + first'(i).  n == 0 gives an empty sketch.
 *   3. Frequency.  *threshold is what fa_mapper_freq_threshold of fa_sketch_index(s) would return (INT_MAX: nothing is
 *      ignored); the distinct hashes with at least *threshold records, ascending as unsigned 32-bit, go to the DEVICE array
 *      d_drop_keys and their number to *n_drop (0 at INT_MAX).  No index is built: at most 2^32 - 1 records
 *      (FA_ERR_UNSUPPORTED beyond), not the 2^31 of an index.
 * Both flush the pending contigs of s first, as fa_sketch_get_minimizers_device does, and otherwise only read it: s holds
 * the same records afterwards and indexes to the same mapper.  The cost of fa_sketch_select goes with the selected records,
 * not with the records of s.  FA_ERR_INVALID from fa_sketch_select: an entry outside [0, n_genomes), a list that does not
 * ascend strictly, contigs behind the last fa_sketch_end_genome of s; *out is then untouched.  A `cap` below the number of
 * keys is FA_ERR_INVALID from fa_sketch_frequency: nothing is written, and *n_drop holds the number needed (as
 * fa_screen_pairs does).  Both run on the sketch's stream, have finished when they return, and are FA_ERR_NO_DEVICE without
 * a device like every compute entry point. */
int fa_sketch_select(fa_sketch *s, const int32_t *genomes, int32_t n, fa_sketch **out);
int fa_sketch_frequency(fa_sketch *s, int *threshold, int64_t cap, uint32_t *d_drop_keys, int64_t *n_drop);

/* ---- Mapper: query side ------------------------------------------------ */
void fa_mapper_free(fa_mapper *m);
/* Sketch_t::getFreqThreshold, include/fastani/map/win_sketch.pxd:40 */
int fa_mapper_freq_threshold(fa_mapper *m, int *threshold);
/* len(Mapper.lookup_index) = minimizerPosLookupIndex.size(), _fastani.pyx:1454-1456 */
int fa_mapper_lookup_size(fa_mapper *m, int64_t *n);
/* The HIP device the mapper's index lives on (fa_set_device at the time Sketch.index() ran; -1: the calling thread's
 * current device).  No reference counterpart (the reference has no device); used by the multi-GPU layer to allocate the
 * tensors it hands to fa_mapper_lookup_export_device / fa_mapper_set_global_frequency on the right GPU. */
int fa_mapper_device(fa_mapper *m, int *device);
/* Reference-sharded index ("when the index does not fit"): every rank indexes its own share of
 * the reference genomes, and the frequency threshold of Sketch_t::computeFreqHist / the `size < threshold` filter of
 * _fastani.pyx:946 must then be taken over the position lists of ALL shards.  fa_mapper_lookup_export_device copies
 * the distinct hashes of this shard (ascending) and their list lengths into caller-owned HBM buffers (e.g. torch
 * tensors, `cap` >= fa_mapper_lookup_size) for the exchange; fa_mapper_set_global_frequency installs the threshold
 * computed over all shards and the hashes (device array) whose summed list length reaches it: the lookup ignores
 * them from then on although their local lists are short.  Call it before the first query on this mapper. */
int fa_mapper_lookup_export_device(fa_mapper *m, int64_t cap, uint32_t *d_keys, int32_t *d_counts);
int fa_mapper_set_global_frequency(fa_mapper *m, int threshold, int64_t n_drop, const uint32_t *d_drop_keys);
/* MinimizerIndex.__iter__/__getitem__, _fastani.pyx:1458-1475 */
int fa_mapper_lookup_keys(fa_mapper *m, uint32_t *keys);
int fa_mapper_lookup_count(fa_mapper *m, uint32_t hash, int64_t *count); /* -1 when absent */
int fa_mapper_lookup_get(fa_mapper *m, uint32_t hash, int32_t *seq_id, int32_t *wpos, int64_t cap);
int fa_mapper_num_minimizers(fa_mapper *m, int64_t *n);
int fa_mapper_get_minimizers(fa_mapper *m, uint32_t *hash, int32_t *seq_id, int32_t *wpos);
int fa_mapper_num_genomes(fa_mapper *m, int64_t *n);
int fa_mapper_get_state(fa_mapper *m, uint64_t *lengths, int32_t *sequences_by_file);
/* The numbering of the reference bins computeCGI keeps one mapping per (query genome, reference genome) for: *bin_length =
 * max(fragment_length - 20, 1), *n_contigs the contigs of the index, contig_bin [n_contigs + 1] the first bin of every contig
 * and contig_genome [n_contigs] its reference genome -- the index's own arrays, downloaded.  A mapping on contig c at
 * ref_start_pos p lies in bin contig_bin[c] + p / bin_length; contig_bin[n_contigs] is the number of bins of the index.  A
 * contig has the bins up to that of its last minimizer window, so a contig WITHOUT minimizer records (shorter than a window)
 * has NO bins: contig_bin[c + 1] == contig_bin[c].  The two arrays may be NULL to ask for the sizes only; bin_length and
 * n_contigs may not. */
int fa_mapper_reference_bins(fa_mapper *m, int32_t *bin_length, int64_t *n_contigs, int32_t *contig_bin, int32_t *contig_genome);

/* Mapper._query_draft up to and including computeCGI, _fastani.pyx:1006-1118, for ONE query genome given as
 * host buffers.  rows receive one cgi::CGI_Results per reference genome with at least one mapping, in
 * refGenomeId order; the minimum_fraction filter and the sort (_fastani.pyx:1121-1136) stay with the caller,
 * which owns the names.  *n_short = contigs skipped with the short-sequence warning (:1061-1070).
 * Re-entrant like the reference's query (:1158-1161): every call borrows one of the mapper's workspaces (a HIP stream
 * and every intermediate buffer), so calls from several host threads on ONE mapper overlap on the device; the stage
 * getters and fa_mapper_last_timings below report the most recently finished call. */
int fa_mapper_query(fa_mapper *m, const void *const *contigs, const int64_t *lengths, int n_contigs, int char_width,
                    fa_cgi_row *rows, int64_t cap, int64_t *n_rows, int *n_short, uint64_t *total_fragments,
                    uint64_t *total_length);

/* fa_mapper_query that also returns the mappings behind its rows: one fa_hit_mapping per (reference genome, reference
 * bin) that computeCGI kept, in (ref_genome_id, bin) order -- the order in which the row's identities are summed.  A pair
 * holds at most one record per query fragment, so total_fragments x reference genomes is a safe map_cap.  A smaller
 * buffer is an error (FA_ERR_INVALID, nothing is written beyond map_cap).  *n_maps then holds the records up to and
 * including the pass that did not fit -- the count of the call only if the call is one pass;
 * fa_mapper_query_mappings_stream with a null sink gives the count of the whole call. */
int fa_mapper_query_mappings(fa_mapper *m, const void *const *contigs, const int64_t *lengths, int n_contigs, int char_width,
                             fa_cgi_row *rows, int64_t cap, int64_t *n_rows, int *n_short, uint64_t *total_fragments,
                             uint64_t *total_length, fa_hit_mapping *maps, int64_t map_cap, int64_t *n_maps);

/* The mappings as a stream: the records leave the device in windows of at most S records (the mapping stage,
 * fa_mapper_set_mapping_stage) through two buffers of S records in HBM and two in pinned host memory that belong to the
 * workspace and do not grow with the table.  `sink` is called once per window, in order, from the calling thread, with
 * every window of a pass full except its last; the records of consecutive passes follow one another in the order of the
 * buffer entry points, and a pass without records calls nothing.  `records` is valid during the call only.  A non-zero
 * return ends the query with FA_ERR_INVALID; the mapper stays usable.  sink == NULL counts: no record is written anywhere
 * and *n_maps is the number of records of the whole call, over all its passes. */
typedef int (*fa_mapping_sink)(void *user, const fa_hit_mapping *records, int64_t n);
int fa_mapper_query_mappings_stream(fa_mapper *m, const void *const *contigs, const int64_t *lengths, int n_contigs, int char_width,
                                    fa_cgi_row *rows, int64_t cap, int64_t *n_rows, int *n_short, uint64_t *total_fragments,
                                    uint64_t *total_length, fa_mapping_sink sink, void *user, int64_t *n_maps);
/* records per stage buffer (>= 1) of the mapping calls that follow; the default is FA_MAP_STAGE_MB (64) megabytes' worth */
int fa_mapper_set_mapping_stage(fa_mapper *m, int64_t records);
/* The rules of the mapper (fa_rules above).  fa_mapper_set_rules: FA_ERR_INVALID for a null pointer or a value outside the
 * ones listed, and the mapper is unchanged.  Takes the mapper lock; a query call follows the rules that were in force when it
 * started, the calls that start afterwards the new ones; setting the rules the mapper already has does nothing.  The index
 * does not depend on the rules.  l2_confidence reaches the percentage_identity filter of doL2Mapping only:
 * estimateMinimumHitsRelaxed and fa_recommended_window_size stay at 0.9. */
int fa_rules_default(fa_rules *out);
int fa_mapper_set_rules(fa_mapper *m, const fa_rules *r);
int fa_mapper_get_rules(fa_mapper *m, fa_rules *out);
/* of the workspace the last mapping call used: records per stage buffer, bytes of its HBM stage, bytes of its pinned stage
 * (both 0 while no call has sent records to the host), bytes of its winner table */
int fa_mapper_mapping_memory(fa_mapper *m, int64_t out[4]);

/* ---- host ingest: FASTA files ------------------------------------------ */
/* Record reader with the semantics of pyfastani._fasta.Parser (src/pyfastani/_fasta.pyx:41-103): records exist only
 * if the first line starts with '>'; id = header line without '>' and newline; sequence lines joined, ASCII letters
 * upper-cased (copy_upper); a header that does not end in '\n' within 2047 bytes fails with FA_ERR_BUFFER.  The
 * pointers returned by fa_fasta_next stay valid until the next call on the same handle. */
typedef struct fa_fasta fa_fasta;
int fa_fasta_open(const char *path, fa_fasta **out);                          /* Parser.__cinit__, _fasta.pyx:49-58 */
int fa_fasta_next(fa_fasta *f, int *has_record, const char **id, int64_t *id_length, const unsigned char **seq,
                  int64_t *seq_length);                                         /* Parser.__next__, _fasta.pyx:66-103 */
void fa_fasta_close(fa_fasta *f);
/* Parser + Sketch._add_draft (_fastani.pyx:610-690) in one native call: every record of the file is a contig of ONE
 * reference genome; records are split and upper-cased by host threads and packed without passing through Python. */
int fa_sketch_add_fasta(fa_sketch *s, const char *path, int64_t *n_records, int64_t *n_short);
/* n_genomes reference genomes from host buffers in ONE call: contig c belongs to genome contig_genome[c] (non-decreasing,
 * < n_genomes; a genome may have no contig); equivalent to fa_sketch_add_contig for every contig and fa_sketch_end_genome
 * for every genome (_fastani.pyx:610-690 per genome), with one run of the packer over all contigs.  n_short: [n_genomes]
 * contigs skipped with the short-sequence warning, or NULL. */
int fa_sketch_add_genomes(fa_sketch *s, const void *const *contigs, const int64_t *lengths, const int32_t *contig_genome,
                          int64_t n_contigs, int32_t n_genomes, int char_width, int32_t *n_short);
/* The same for n_paths reference genomes, one per file, in the order given: the files are read and 2-bit packed
 * concurrently (one host task per file, straight from the file's bytes to packed words), then added as n_paths
 * consecutive fa_sketch_add_fasta calls would have added them.  n_records / n_short: [n_paths] or NULL.  The host side
 * of the reference's benchmark loop `for path: sketch.add_draft(name, [r.seq for r in Parser(path)])`
 * (benches/mapping/bench.py:41-47). */
int fa_sketch_add_fasta_many(fa_sketch *s, const char *const *paths, int32_t n_paths, int64_t *n_records, int64_t *n_short);
/* One query genome per FASTA file, packed and uploaded as a resident batch (fa_genomes_upload semantics); the files
 * are read concurrently, and the upload runs on a stream of the batch's own. */
int fa_genomes_upload_fasta(fa_mapper *m, const char *const *paths, int32_t n_paths, fa_genomes **out);
/* FASTA files read and 2-bit packed ONCE (one genome per file, the files concurrently), to be used as references and as
 * queries: an all-vs-all -- the reference benchmark's shape, benches/mapping/bench.py:41-53: the genomes that are sketched are
 * the genomes that are mapped -- reads every file one time.  protein != 0: residue bytes are kept instead. */
typedef struct fa_packed fa_packed;
int fa_packed_read(const char *const *paths, int32_t n_paths, int protein, fa_packed **out);
/* more files behind the ones it holds.  Thread-safe against the calls that read the set (info, add_packed, reload_packed): it
 * grows the set under an exclusive lock they hold shared; fa_packed_free must not race with any of them. */
int fa_packed_append(fa_packed *p, const char *const *paths, int32_t n_paths);
void fa_packed_free(fa_packed *p);
/* per file: its size in bytes, its records, its bases (arrays of *n_files entries, any may be NULL) */
int fa_packed_info(fa_packed *p, int32_t *n_files, uint64_t *file_bytes, int64_t *records, int64_t *bases);
/* files [first, first + count) as that many reference genomes (fa_sketch_add_fasta_many without reading) */
int fa_sketch_add_packed(fa_sketch *s, fa_packed *p, int32_t first, int32_t count, int64_t *n_records, int64_t *n_short);
/* files [first, first + count) as the query genomes of a recycled batch (fa_genomes_reload_fasta without reading) */
int fa_genomes_reload_packed(fa_mapper *m, fa_genomes *g, fa_packed *p, int32_t first, int32_t count);
/* Refills a batch from other files, recycling its device buffers, its pinned staging image and its stream: the
 * double-buffered form for a stream of query chunks (while one batch is mapped by fa_mapper_query_genomes on one host
 * thread, another thread refills the other batch).  A failed refill leaves an empty batch. */
int fa_genomes_reload_fasta(fa_mapper *m, fa_genomes *g, const char *const *paths, int32_t n_paths);

/* ---- resident batches (many-to-many; inputs stay in HBM) -------------- */
/* Pack + upload a batch of query genomes.  contig_genome[i] is the genome (0..n_genomes-1, non-decreasing)
 * contig i belongs to.  Short contigs are skipped exactly as _fastani.pyx:1061-1070 does. */
int fa_genomes_upload(fa_mapper *m, const void *const *contigs, const int64_t *lengths, const int32_t *contig_genome,
                      int64_t n_contigs, int32_t n_genomes, int char_width, fa_genomes **out);
void fa_genomes_free(fa_genomes *g);
int fa_genomes_info(fa_genomes *g, int32_t *n_genomes, uint64_t *total_fragments, uint64_t *total_length,
                    int32_t *n_short); /* arrays of n_genomes entries, may be NULL */
/* Map genomes [first, first+count) of a resident batch against the resident index: the hot path
 * (K1 sketch -> lookup -> L1 -> L2 -> CGI), everything on device.  rows as fa_mapper_query, query_id = index in
 * the batch.  If rows_device is non-zero, `rows` is a DEVICE pointer (e.g. a torch tensor feeding an RCCL
 * all-gather) with room for `cap` rows. */
int fa_mapper_query_genomes(fa_mapper *m, fa_genomes *g, int32_t first, int32_t count, fa_cgi_row *rows, int64_t cap,
                            int64_t *n_rows, int rows_device);

/* fa_mapper_query_genomes that also returns the mappings behind its rows, in (query_id, ref_genome_id, bin) order; the
 * records of consecutive passes follow one another.  A safe map_cap is the number of query fragments of the range
 * (fa_genomes_info) times the number of reference genomes; a smaller buffer is an error (FA_ERR_INVALID, nothing is
 * written beyond map_cap).  *n_maps then holds the records up to and including the pass that did not fit, which is the
 * count of the call only if the call is one pass: fa_mapper_query_genomes_mappings_stream with a null sink counts the whole
 * call, and with a sink needs no bound at all.  A host destination is filled through the workspace's mapping stage (see
 * fa_mapper_query_mappings_stream): the library holds no device buffer of map_cap records.  The workspace keeps a winner
 * table of 16 bytes per (query of a pass, reference bin).  If maps_device is non-zero, `maps` is a DEVICE pointer with room
 * for map_cap records, as `rows` is under rows_device, and every pass writes its records straight into it.  The winner
 * table, the stage and the compaction behind these records exist only in calls through the mapping entry points:
 * fa_mapper_query_genomes launches and allocates what it always did. */
int fa_mapper_query_genomes_mappings(fa_mapper *m, fa_genomes *g, int32_t first, int32_t count, fa_cgi_row *rows, int64_t cap,
                                     int64_t *n_rows, int rows_device, fa_hit_mapping *maps, int64_t map_cap,
                                     int64_t *n_maps, int maps_device);
int fa_mapper_query_genomes_mappings_stream(fa_mapper *m, fa_genomes *g, int32_t first, int32_t count, fa_cgi_row *rows, int64_t cap,
                                            int64_t *n_rows, int rows_device, fa_mapping_sink sink, void *user, int64_t *n_maps);

/* ---- the hit table of an all-vs-all, reduced on the device ------------- */
/* What an all-vs-all over ONE genome set is run for: the symmetric identity of every genome pair and the groups of genomes
 * above a cut-off (species clusters at 95, dereplication at 99) -- FastANI's matrix output (cgi::outputPhylip,
 * include/fastani/cgi/compute_core_identity.pxd:39-51) and the single-linkage step that follows it.  Genomes are numbered
 * 0 .. n_genomes-1; query_id and ref_genome_id of the rows index the same list.
 *   1. Filter.  A row (q, r) with q == r never forms a pair.  Another row survives iff
 *        (float)((uint64_t)count_seq * fragment_length) >= (float)min(query_lengths[q], reference_lengths[r]) * min_fraction
 *      in float32 (_fastani.pyx:1121-1132).  An id outside [0, n_genomes), or the same (q, r) in two rows of the table, is
 *      FA_ERR_INVALID and nothing is returned.
 *   2. Pair (a, b), a < b: identity_ab is the identity of the surviving row with query a and reference b, identity_ba of the
 *      other direction, a missing direction NaN; identity is the float64 mean of the two when both survive, else the one that
 *      does.  Pairs come out sorted by (a, b), and the same input gives the same bytes on every run.
 *   3. Edge: a pair with identity >= (double)min_identity that, with reciprocal != 0, also has both directions.
 *   4. Clusters: the connected components of the edges.  labels[g] is the smallest genome number in g's component (a genome
 *      without an edge labels itself); *n_clusters is the number of g with labels[g] == g. */
typedef struct fa_pair {
  int32_t a, b;               /* a < b */
  float identity_ab;          /* query a on reference b, NaN when that row is missing or filtered */
  float identity_ba;          /* query b on reference a */
  double identity;            /* the symmetric value */
} fa_pair;                    /* 24 bytes */
typedef struct fa_table_params {
  float min_fraction;         /* minFraction of the filter */
  int32_t fragment_length;    /* minReadLength the rows were mapped with (>= 1) */
  float min_identity;         /* the cut-off of an edge (fa_table_clusters, fa_table_representatives) */
  int32_t reciprocal;         /* != 0: an edge needs both directions (fa_table_clusters, fa_table_representatives) */
} fa_table_params;            /* 16 bytes */
/* All pairs of the table (not only the edges).  rows_device / pairs_device != 0: `rows` / `pairs` are DEVICE pointers, as on
 * fa_mapper_query_genomes; the two length arrays (n_genomes entries each) are host memory.  pairs == NULL only counts.  A `cap`
 * below the number of pairs is FA_ERR_INVALID: nothing is written, and *n_pairs holds the number needed (a table of n_rows
 * rows has at most n_rows pairs).  Runs on the calling thread's current device, on a stream of its own, with memory from the
 * device pool, and has finished when it returns; without a device it fails with FA_ERR_NO_DEVICE like every compute entry. */
int fa_table_pairs(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes, const uint64_t *query_lengths,
                   const uint64_t *reference_lengths, const fa_table_params *p, fa_pair *pairs, int64_t cap, int64_t *n_pairs,
                   int pairs_device);
/* The clusters of the table: labels [n_genomes] (a DEVICE pointer when labels_device != 0).  n_clusters and stats may be
 * NULL; stats[0] surviving rows, [1] pairs, [2] edges, [3] rounds of the component loop (the round that found nothing to
 * lower included; 0 without an edge). */
int fa_table_clusters(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes, const uint64_t *query_lengths,
                      const uint64_t *reference_lengths, const fa_table_params *p, int32_t *labels, int labels_device,
                      int32_t *n_clusters, int64_t *stats);
/* Greedy representative clustering of the table (GTDB species clusters, dRep's and galah's dereplicated sets): unlike the
 * connected components, every genome is within the cut-off of the genome that stands for it.
 *   1. Filter, pair, edge: steps 1-3 above, `reciprocal` included.  min_identity must be a number >= 0 (a negative or NaN
 *      value is FA_ERR_INVALID, as in fa_best_params), so every edge's identity is >= 0; -0.0 is treated as +0.0.
 *   2. Order.  `order` is a HOST array of n_genomes int32, a permutation of the genome numbers; order[0] is the most preferred
 *      genome, NULL means genome-number order.  pos[g] is the place of g in `order`.  Anything that is not a permutation (a
 *      value outside [0, n_genomes), a value that occurs twice) is FA_ERR_INVALID with nothing written.
 *   3. Representatives.  Walk the genomes in `order`: a genome is a representative iff it has no edge to a representative with
 *      a smaller pos.  Equivalently R is the one set with  g in R  <=>  no edge neighbour h with pos[h] < pos[g] is in R.
 *   4. Assignment.  labels[g] = g for a representative.  Any other genome has at least one neighbour that is a
 *      representative and gets the one with the largest symmetric identity, compared as float64 (not float32), ties to the
 *      smaller pos.  identity[g] is that pair's symmetric identity, 100.0 for a representative.  *n_representatives is the
 *      number of g with labels[g] == g.  The same input gives the same bytes on every run.
 * labels [n_genomes] int32 and identity [n_genomes] float64 (may be NULL) are DEVICE pointers when out_device != 0.
 * n_representatives and stats may be NULL; stats[0] surviving rows, [1] pairs, [2] edges, [3] rounds of the selection loop (at
 * most n_genomes; 0 without an edge).  Everything else as for fa_table_clusters: a bad id or a duplicate row is
 * FA_ERR_INVALID with nothing written, the out-parameters included; the call runs on the calling thread's current device, on
 * a stream of its own, with memory from the device pool, has finished when it returns, and is FA_ERR_NO_DEVICE without a
 * device. */
int fa_table_representatives(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes,
                             const uint64_t *query_lengths, const uint64_t *reference_lengths, const fa_table_params *p,
                             const int32_t *order, int32_t *labels, double *identity, int out_device,
                             int32_t *n_representatives, int64_t *stats);
/* Average-linkage (UPGMA) clusters of the table at one cut-off -- dRep's default for both of its steps, and what is run on
 * FastANI's matrix output with scipy's linkage(method="average") and fcluster(criterion="distance"): unlike the connected
 * components it does not chain, and unlike the representatives it does not depend on an order the caller brings.
 *   1. Filter and pair: steps 1-2 above.  A pair is PRESENT iff it exists after the filter and, with reciprocal != 0, has
 *      both directions.
 *   2. Weight.  A present pair's weight is w = rint(identity * 2^20) as int64, ties to even, identity being the pair's float64
 *      symmetric identity: exact for what FastANI reports (a float32 at or above 16 is a multiple of 2^-19, a mean of two a
 *      multiple of 2^-20).  `missing` is the identity assumed for every pair that is not present (dRep: 0; or the floor
 *      below which FastANI reports nothing): qm = rint((double)missing * 2^20).  qc = rint((double)min_identity * 2^20).
 *   3. State.  A cluster's label is its smallest genome number; every genome starts alone.  For two clusters A and B, c(A,B)
 *      is the number of present pairs between them, S(A,B) = sum of their w + qm * (|A||B| - c(A,B)), and the average is
 *      S(A,B) / (|A||B|).  Only cluster pairs with c > 0 are candidates.
 *   4. Order.  Candidate (A,B) comes before (C,D) iff its average is larger, compared exactly as S(A,B) * |C||D| against
 *      S(C,D) * |A||B| in integers (128 bits; never float64); ties go to the smaller min(label), then to the smaller max(label).
 *   5. Merge.  While the first candidate in that order has S >= qc * |A||B|, merge it: sums and counts add, the label is the
 *      smaller one.
 *   6. Result.  labels[g] is the label of g's cluster, *n_clusters the number of g with labels[g] == g.  The same input gives
 *      the same bytes on every run.  (The library merges every mutual first pair of a round at once; the labels are those of
 *      the sequential walk.)
 *   7. FA_ERR_INVALID with nothing written, the out-parameters included: everything fa_table_clusters rejects; min_identity
 *      or missing negative or NaN; missing >= min_identity, compared as qm >= qc; a present pair whose identity is NaN or
 *      outside [0, 128].  n_genomes > 2^18 is FA_ERR_UNSUPPORTED: S stays below 2^62 and the cross products below 2^128.
 * labels [n_genomes] is a DEVICE pointer when labels_device != 0.  n_clusters and stats may be NULL; stats[0] surviving rows,
 * [1] pairs, [2] present pairs, [3] rounds (those that merged a pair: at most n_genomes - 1; a block of exactly tied genomes
 * merges one pair per round), [4] merges = n_genomes - *n_clusters.  Runs like fa_table_clusters: on the calling thread's
 * current device, on a stream of its own, with memory from the device pool, finished when it returns, FA_ERR_NO_DEVICE
 * without a device.  Only the partition at one cut-off is returned; fa_table_dendrogram returns the merge list, the tree,
 * as well. */
int fa_table_linkage(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes, const uint64_t *query_lengths,
                     const uint64_t *reference_lengths, const fa_table_params *p, float missing, int32_t *labels, int labels_device,
                     int32_t *n_clusters, int64_t *stats);
/* One merge of the sequential walk of step 5. */
typedef struct fa_merge {
  int32_t lo, hi;            /* labels of the two clusters before the merge, lo < hi; the merged cluster is labelled lo */
  int32_t size_lo, size_hi;  /* their sizes before the merge; n = size_lo * size_hi */
  int64_t s;                 /* S(A,B) of step 3: sum of w + qm * (n - present) */
  int64_t present;           /* c(A,B): present genome pairs between them, >= 1 */
} fa_merge;                  /* 32 bytes */
/* The average-linkage dendrogram of the table: every merge of fa_table_linkage's walk, so that the partition at any cut-off
 * at or above the one it was built with is had without another pass over the table (fa_dendrogram_cut).  Steps 1-7 of
 * fa_table_linkage apply word for word, stats[0..4] included.  p->min_identity is the BUILD cut-off: the tree is known down
 * to it (for the whole tree pass any value just above `missing`).
 *   merges    receives every merge of the sequential walk, in the order of the walk -- which is the order of step 4 applied
 *             to {s, size_lo * size_hi, lo, hi}: the walk visits its merges in that order (average linkage is reducible),
 *             so the merges that pass a cut-off t >= the build cut-off are a prefix of the list, and that prefix is the walk
 *             of fa_table_linkage at t.  *n_merges (not NULL) is their number, equal to stats[4]; a table has at most
 *             n_genomes - 1.  merges == NULL only counts.  A `cap` below the number of merges is FA_ERR_INVALID with nothing
 *             written but *n_merges.
 *   labels    may be NULL; otherwise [n_genomes], the partition at the build cut-off, byte for byte what fa_table_linkage
 *             returns for the same arguments.
 * out_device != 0: `merges` and `labels` are both DEVICE pointers.  n_clusters and stats may be NULL.  The same input gives
 * the same bytes on every run. */
int fa_table_dendrogram(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes, const uint64_t *query_lengths,
                        const uint64_t *reference_lengths, const fa_table_params *p, float missing, fa_merge *merges, int64_t cap,
                        int64_t *n_merges, int32_t *labels, int out_device, int32_t *n_clusters, int64_t *stats);
/* The partitions of a merge list at n_cuts >= 1 cut-offs.  min_identity is a HOST array of n_cuts values; for cut t, qc is
 * formed exactly as in fa_table_linkage (rint of the value times 2^20, clamped just above the largest weight), and merge i
 * applies iff s >= qc * size_lo * size_hi.  labels is laid out [n_cuts][n_genomes] (a DEVICE pointer when labels_device != 0,
 * as `merges` is when merges_device != 0): labels[t][g] is the root of g in the forest parent[hi] = lo over the applying
 * merges -- for a list of fa_table_dendrogram the smallest member of g's cluster, as everywhere else.  n_clusters, a HOST
 * array of n_cuts values, may be NULL.  The call cannot know the cut-off a list was built with: a cut below it returns the
 * build partition (the list ends there), so keep the build cut-off with the list (pyfastani_amd.clusters.Dendrogram does,
 * and refuses such a cut).  FA_ERR_INVALID with nothing written: a negative or NaN cut; n_cuts < 1; n_merges outside
 * [0, max(n_genomes - 1, 0)]; a merge with lo < 0, lo >= hi or hi >= n_genomes; a hi that occurs in two merges; a size
 * below 1, or two sizes that add up to more than n_genomes; s < 0; present < 1.  More than 2^18 genomes, or more than
 * 2^31 - 1 labels in all, are FA_ERR_UNSUPPORTED.  Runs like the other reductions: on the calling thread's current device, on
 * a stream of its own, with memory from the device pool, finished when it returns, FA_ERR_NO_DEVICE without a device.  The
 * same input gives the same bytes on every run. */
int fa_dendrogram_cut(const fa_merge *merges, int64_t n_merges, int merges_device, int32_t n_genomes, const float *min_identity,
                      int32_t n_cuts, int32_t *labels, int labels_device, int32_t *n_clusters);
/* The order of step 4 on two candidates a and b = {S, |A||B|, lo, hi} (S >= 0, |A||B| >= 1, labels >= 0, else
 * FA_ERR_INVALID): *first = 1 when a comes before b, 0 when b comes before a, 2 when they are equal.  Host only; it calls the
 * comparator the kernels use. */
int fa_debug_linkage_order(const int64_t a[4], const int64_t b[4], int *first);
/* Centrality and medoids of given clusters of the table: for every genome its mean identity to the other members of its
 * cluster, and for every cluster the member that stands for it (dRep's score = quality + centrality), whichever rule made the
 * partition.  Several partitions -- the cuts of a dendrogram -- are served by one pass over the table.
 *   1. Filter, pair, present, weight: steps 1-2 of fa_table_linkage word for word, `reciprocal` included.  w = rint(identity *
 *      2^20), qm = rint((double)missing * 2^20).  p->min_identity is not read: the labels carry the cut-off.
 *   2. Labels.  labels is laid out [n_sets][n_genomes], n_sets >= 1.  A set t is valid iff every labels[t][g] lies in
 *      [0, n_genomes) and labels[t][labels[t][g]] == labels[t][g]: every label is a member of its own cluster, as in what
 *      fa_table_clusters, fa_table_linkage, fa_dendrogram_cut and fa_table_representatives return.  The cluster of g in set t
 *      is {h : labels[t][h] == labels[t][g]}; m is its size.
 *   3. Centrality.  S[t][g] = sum of w(g,h) over the present pairs with h != g in g's cluster + qm * (m - 1 - their number).
 *      The mean identity of g to its cluster is S / (m - 1); for m == 1, S = 0.  With at most 2^18 genomes S < 2^46.
 *   4. Bonus.  bonus is a HOST array [n_genomes], NULL meaning all zero: the caller's quality score in identity points.
 *      qb[g] = rint(bonus[g] * 2^20), |bonus[g]| <= 32768, and T[t][g] = S[t][g] + qb[g] * (m - 1): "mean centrality + bonus",
 *      compared exactly in int64 (|T| < 2^54).
 *   5. Medoid.  The medoid of a cluster is its member with the largest T, ties to the smaller genome number.  medoids[t][g] is
 *      the medoid of g's cluster in set t; n_clusters, a HOST array [n_sets] that may be NULL, counts the g with
 *      medoids[t][g] == g.
 *   6. Identity.  identity[t][g] is 100.0 when g is its own medoid; w / 2^20 as float64 for the present pair (g, medoid); NaN
 *      (0x7ff8000000000000) when that pair is not present -- under average linkage a member need not have a row with its
 *      medoid.  w / 2^20 equals the pair's symmetric identity whenever that is a multiple of 2^-20, which holds for
 *      everything FastANI reports at or above 16.
 *   7. Outputs.  sums and sizes, [n_sets][n_genomes], hold S and m.  medoids, identity, sums and sizes may each be NULL.
 *      labels and all four outputs are DEVICE pointers when io_device != 0.
 *   8. stats may be NULL; stats[0] surviving rows, [1] pairs, [2] present pairs, [3] present pairs that lie inside a cluster,
 *      summed over the sets.
 *   9. FA_ERR_INVALID with nothing written, the out-parameters included: everything fa_table_clusters rejects; missing
 *      negative, NaN or above 128; n_sets < 1; null labels with n_genomes > 0; an invalid label set; a bonus that is NaN or
 *      beyond +-32768; a present pair whose identity is NaN or outside [0, 128].  n_genomes > 2^18, or n_sets * n_genomes >
 *      2^31 - 1, is FA_ERR_UNSUPPORTED.
 *  10. Runs like the other reductions: on the calling thread's current device, on a stream of its own, with memory from the
 *      device pool, finished when it returns, FA_ERR_NO_DEVICE without a device.  The same input gives the same bytes on
 *      every run. */
int fa_table_medoids(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_genomes, const uint64_t *query_lengths,
                     const uint64_t *reference_lengths, const fa_table_params *p, float missing, const int32_t *labels, int32_t n_sets,
                     const double *bonus, int32_t *medoids, double *identity, int64_t *sums, int32_t *sizes, int io_device,
                     int32_t *n_clusters, int64_t *stats);
/* Steps 4-5 on two members b and a of one cluster of m genomes (1 <= m <= 2^18; S in [0, 2^46), |bonus| <= 32768, numbers >= 0,
 * else FA_ERR_INVALID): t[0] = T of b, t[1] = T of a, *better = 1 when b replaces a as the medoid, else 0.  Host only; it calls
 * the functions the kernels use. */
int fa_debug_medoid_better(double bonus_b, int64_t s_b, int32_t b, double bonus_a, int64_t s_a, int32_t a, int32_t m, int64_t t[2],
                           int *better);

/* ---- the fragment mappings behind a hit table, reduced to a per-fragment profile ---- */
/* What a mapping table is read for: which parts of a genome are shared with its relatives, and how well -- the per-fragment
 * reading of core-genome identity.  The records (fa_hit_mapping, left in HBM by fa_mapper_query_genomes_mappings with
 * maps_device) are accumulated call by call into one entry per query fragment, and the entries reduced per genome.
 *   1. Profile.  Over a batch of n_queries query genomes, fragment_offsets [n_queries + 1] is the prefix sum of the genomes'
 *      fragment numbers (fa_genomes_info's total_fragments), fragment_offsets[0] == 0; fragment f (= query_seq_id) of query q
 *      is entry fragment_offsets[q] + f.  An entry holds count (int32), the number of counted records; sum (int64), the sum
 *      of their identities in fixed point, rint(identity * 2^20), ties to even; lowest (float32), the smallest identity among
 *      them, +inf while count == 0.  The three arrays are the caller's DEVICE memory, fragment_offsets[n_queries] entries
 *      each, initialised by the caller (0, 0, +inf) and owned by it across calls.
 *   2. Counted.  A record (q, f, r, identity) is counted iff identity >= min_identity in float32 (equality counts), and,
 *      with labels, query_labels[q] == reference_labels[r], and, with self_reference, self_reference[q] != r:
 *      self_reference[q] is the reference number that is query q itself, -1 for none -- how an all-vs-all drops its diagonal
 *      and a chunked batch says which global genome each query is.  query_labels [n_queries], reference_labels
 *      [n_references] and self_reference [n_queries] are HOST arrays, each NULL for none; the two label arrays go together.
 *   3. Order.  All three accumulators are integers, or the orderable bit pattern of a non-negative float: the result does
 *      not depend on the order of the records, on how they are split over calls, or on the road the kernel takes.
 *      Accumulating one pass and then the next gives the bytes of one call over both.
 *   4. stats may be NULL; [0] records counted, [1] records at or above min_identity that labels or self dropped, [2] records
 *      below min_identity, [3] workgroups of the accumulate kernel that summed on chip before touching HBM.
 *   5. FA_ERR_INVALID with the accumulators untouched: a query_id outside [0, n_queries); a query_seq_id outside [0, the
 *      fragments of its query); a ref_genome_id outside [0, n_references); an identity that is NaN, has its sign bit set
 *      (-0.0 included: the minimum is taken on the bit pattern) or lies above 128; offsets that do not start at 0 or that
 *      decrease; a negative count; one label array without the other; a NaN min_identity; NULL accumulators with a fragment
 *      to hold.  n_maps == 0 is valid and touches nothing.
 *   6. Not checked: the same (query, fragment, reference) in two records.  The mapper never emits that, and across calls it
 *      cannot be seen; such a record counts twice.
 *   7. What the records are.  They are the mappings computeCGI KEPT: the best of a query fragment per reference genome, then
 *      the best per reference bin.  A fragment that lost its reference bin to a neighbour is absent from that reference's
 *      records: count is "references whose hit counts this fragment", not "references where it would map".
 * `maps` is a DEVICE pointer when maps_device != 0.  Runs like the table reductions: on the calling thread's current device,
 * on a stream of its own, with memory from the device pool, finished when it returns, FA_ERR_NO_DEVICE without a device. */
int fa_mappings_profile(const fa_hit_mapping *maps, int64_t n_maps, int maps_device, int32_t n_queries, const int64_t *fragment_offsets,
                        int32_t n_references, const int32_t *query_labels, const int32_t *reference_labels, const int32_t *self_reference,
                        float min_identity, int32_t *d_count, int64_t *d_sum, float *d_lowest, int64_t *stats);
/* The summary of a profile.  min_count is a HOST array [n_sets][n_queries], every value >= 0, n_sets >= 1.  For every
 * (set, q), over the fragments of q with count >= min_count[set][q]: fragments, how many there are; hits, the sum of their
 * counts; sum, the sum of their fixed-point sums.  From these and the genome's fragment number the caller forms the core
 * fraction at a presence threshold, the whole presence curve (one set per threshold) and the mean identity of the core,
 * sum / hits / 2^20.  A genome without fragments gives zeros.  d_count and d_sum are DEVICE pointers; the three outputs, each
 * [n_sets][n_queries] and each of which may be NULL, are DEVICE pointers when out_device != 0.  FA_ERR_INVALID with nothing
 * written: n_sets < 1, a negative min_count, bad offsets as above, NULL min_count or accumulators where there is something
 * to read.  n_sets * n_queries > 2^31 - 1 is FA_ERR_UNSUPPORTED. */
int fa_profile_summary(const int32_t *d_count, const int64_t *d_sum, int32_t n_queries, const int64_t *fragment_offsets,
                       const int32_t *min_count, int32_t n_sets, int64_t *fragments, int64_t *hits, int64_t *sum, int out_device);
/* The two constants of the accumulate kernel: the records a workgroup takes, and the most fragments a query may have for a
 * workgroup whose records all belong to it to sum on chip; host only. */
int fa_profile_chunk(int32_t *records_per_workgroup, int32_t *lds_fragments);
/* development: the road of the accumulate kernel for the process -- 0 the policy, 1 always global atomics, 2 on chip wherever
 * it fits; the results do not depend on it (scripts/time_fragment_profile.py times both); host only */
int fa_debug_profile_road(int32_t road);

/* ---- the same records, reduced by reference position; and the regions of either profile ---- */
/* The other half of the reading: which parts of a REFERENCE the queries share, and where its islands are.  The key space is
 * the mapper's own (fa_mapper_reference_bins): one entry per reference bin.
 *   1. Profile.  A record goes to entry contig_bin[ref_seq_id] + ref_start_pos / bin_length, the bin computeCGI kept it for.
 *      An entry holds count (int32), sum (int64, rint(identity * 2^20), ties to even) and lowest (float32, +inf while count
 *      == 0), as in fa_mappings_profile.  The three arrays are the caller's DEVICE memory, contig_bin[n_contigs] entries each,
 *      initialised by the caller (0, 0, +inf) and owned by it across calls.  contig_bin [n_contigs + 1] and contig_genome
 *      [n_contigs] are HOST arrays.
 *   2. Counted.  Exactly the rules of fa_mappings_profile: identity >= min_identity in float32 is asked first (equality
 *      counts), then, with labels, query_labels[q] == reference_labels[r], then, with self_reference, self_reference[q] != r.
 *      The three are HOST arrays, each NULL for none; the two label arrays go together.
 *   3. Order.  Every accumulator is an integer atomic -- the minimum on the bit pattern of a non-negative float --, and there
 *      is no float atomic: the bytes do not depend on the order of the records, on how they are split over calls, or on
 *      timing.
 *   4. stats may be NULL; [0] records counted, [1] records at or above min_identity that labels or self dropped, [2] records
 *      below min_identity.
 *   5. FA_ERR_INVALID with the accumulators untouched: everything fa_mappings_profile refuses about query_id, ref_genome_id,
 *      identity, the labels and min_identity; a ref_seq_id outside [0, n_contigs); contig_genome[ref_seq_id] != ref_genome_id;
 *      ref_start_pos < 0, or its bin not below the contig's number of bins, contig_bin[c + 1] - contig_bin[c]; bin_length
 *      < 1; a contig_bin that does not start at 0 or that decreases; a contig_genome that decreases or leaves [0,
 *      n_references); a negative count; NULL accumulators with a bin to hold.  n_maps == 0 is valid and touches nothing.
 *   6. Not read and not checked: query_seq_id.  Not checked: the same (query, reference genome, bin) in two records; the
 *      mapper never emits that, and such a record counts twice.
 *   7. What count means.  The mapper emits at most one record per (query genome, reference genome, bin), so count[bin] is
 *      the number of query genomes whose hit counts a mapping that STARTS in that bin.  Three properties of FastANI's
 *      binning follow, none of them of this code.  (a) Bins are 20 bases shorter than fragments: with identical coordinates
 *      about one bin in fragment_length / 20 holds no fragment start.  (b) A start can slip across a bin boundary: an indel
 *      moves a mapping's start a few bases into the neighbouring bin, which then holds two candidates and keeps one, and the
 *      bin beside it stays empty for that query.  (c) The last bin of a contig never receives a start, because no whole
 *      fragment fits there.  ONE empty bin is therefore no evidence of absence; a run of two or more is, which is what the
 *      min_length of fa_profile_regions is for.
 * `maps` is a DEVICE pointer when maps_device != 0.  Runs like fa_mappings_profile. */
int fa_mappings_reference_profile(const fa_hit_mapping *maps, int64_t n_maps, int maps_device, int32_t n_queries, int32_t n_references,
                                  int32_t n_contigs, const int32_t *contig_bin, const int32_t *contig_genome, int32_t bin_length,
                                  const int32_t *query_labels, const int32_t *reference_labels, const int32_t *self_reference,
                                  float min_identity, int32_t *d_count, int64_t *d_sum, float *d_lowest, int64_t *stats /* [3] */);
/* The records a workgroup of the reference profile's kernels takes; host only. */
int fa_reference_profile_chunk(int32_t *records_per_workgroup);

/* The regions of a profile, of either side: the maximal runs of entries that hold.  A segment is a contig: segment_offsets
 * [n_segments + 1], a HOST array from 0 that never decreases, delimits the entries of every segment -- contig_bin on the
 * reference side; on the query side the prefix sum of contig_length / fragment_length over the contigs of every genome.
 * Entry i of segment s HOLDS iff count[i] >= need[s]; with below != 0, iff count[i] < need[s].  need [n_segments] is a HOST
 * array, every value >= 0.  A region is a maximal run of holding entries inside ONE segment: runs never join across a
 * segment boundary, and runs of fewer than min_length (>= 1) entries are dropped.  A record gives the segment, the run's
 * first entry relative to the segment's start, its length, hits, the sum of count over the run, and sum, the sum of the
 * fixed-point sums over it (0 with d_sum == NULL); reserved is 0.  Records come out in (segment, first) order; the same
 * input gives the same bytes on every run.  d_count and d_sum are DEVICE pointers; `regions` is one when out_device != 0.
 * regions == NULL only counts; n_regions may be NULL.  A `cap` below the number of records is FA_ERR_INVALID: nothing is
 * written to regions and *n_regions holds the number needed.  FA_ERR_INVALID with nothing written anywhere: n_segments < 0,
 * offsets that do not start at 0 or that decrease, a negative need, min_length < 1, a negative cap, NULL need or d_count
 * where there is something to read.  More than 2^31 - 1 entries is FA_ERR_UNSUPPORTED.  Runs like fa_table_best. */
typedef struct fa_profile_region {
  int32_t segment;          /* the contig, as segment_offsets numbers it */
  int32_t first;            /* first entry of the run, relative to the segment's start */
  int32_t length;           /* entries of the run, >= min_length */
  int32_t reserved;         /* 0 */
  int64_t hits;             /* sum of count over the run */
  int64_t sum;              /* sum of the fixed-point sums over the run */
} fa_profile_region;        /* 32 bytes */
int fa_profile_regions(const int32_t *d_count, const int64_t *d_sum, int32_t n_segments, const int64_t *segment_offsets,
                       const int32_t *need, int below, int32_t min_length, fa_profile_region *regions, int64_t cap,
                       int64_t *n_regions, int out_device);
/* The entries a workgroup of the regions' kernels takes; host only. */
int fa_profile_regions_chunk(int32_t *entries_per_workgroup);

/* ---- a query x reference hit table, reduced to every query's k best hits ---- */
/* What a batch of queries is mapped against a reference database for: per query, the closest references that pass an identity
 * and an aligned-fraction cut-off (species assignment: ANI >= 95 with AF >= 0.5; over one genome set with exclude_self, every
 * genome's nearest neighbours).  Queries are numbered 0 .. n_queries-1 and references 0 .. n_references-1; the two lists are
 * unrelated and may differ in length.
 *   1. Survival.  A row (q, r) survives iff all four hold, each evaluated in float32 exactly as written:
 *        not (exclude_self and q == r);
 *        (float)((uint64_t)count_seq * fragment_length) >= (float)min(query_lengths[q], reference_lengths[r]) * min_fraction
 *          (the filter of fa_table_pairs, _fastani.pyx:1121-1132);
 *        the sign bit of identity is clear, it is not NaN, and identity >= min_identity;
 *        (float)count_seq >= (float)total_query_fragments * min_aligned_fraction.
 *   2. Order.  The survivors of a query are ordered by identity descending, ties by ref_genome_id ascending: with k >= the
 *      number of survivors, the order of the hits query_draft returns.
 *   3. Output.  best holds the first min(k, survivors) rows of every query -- queries ascending, a query's rows in rank order,
 *      each a byte-for-byte copy of its input row; offsets [n_queries + 1]: query q's records are best[offsets[q] ..
 *      offsets[q+1]), a query without survivors has an empty range, offsets[n_queries] == *n_best.  The same input gives the
 *      same bytes on every run. */
typedef struct fa_best_params {
  float   min_fraction;          /* minFraction of the hit filter, as in fa_table_params */
  int32_t fragment_length;       /* >= 1 */
  float   min_identity;          /* >= 0, not NaN */
  float   min_aligned_fraction;  /* >= 0, not NaN: count_seq / total_query_fragments */
  int32_t k;                     /* >= 1: records kept per query */
  int32_t exclude_self;          /* != 0: a row with query_id == ref_genome_id never survives */
} fa_best_params;                /* 24 bytes */
/* rows_device != 0: `rows` is a DEVICE pointer; out_device != 0: `best` and `offsets` are; the two length arrays are host
 * memory.  best == NULL only counts (offsets, if given, is still written); offsets, stats and n_best may be NULL.  A `cap`
 * below the number of records is FA_ERR_INVALID: nothing is written to best or offsets, and *n_best holds the number needed
 * (min(n_rows, n_queries * k) always suffices).  FA_ERR_INVALID with nothing written anywhere, *n_best included: a query id
 * outside [0, n_queries) or a reference id outside [0, n_references); the same (q, r) in two rows, surviving or not; k < 1,
 * fragment_length < 1, a negative or NaN min_identity or min_aligned_fraction; a NULL p or NULL lengths.  stats[0] surviving
 * rows, [1] queries with at least one record, [2] records.  Runs like fa_table_pairs: on the calling thread's current
 * device, on a stream of its own, with memory from the device pool, finished when it returns, FA_ERR_NO_DEVICE without a
 * device. */
int fa_table_best(const fa_cgi_row *rows, int64_t n_rows, int rows_device, int32_t n_queries, int32_t n_references,
                  const uint64_t *query_lengths, const uint64_t *reference_lengths, const fa_best_params *p,
                  fa_cgi_row *best, int64_t *offsets, int64_t cap, int64_t *n_best, int out_device, int64_t *stats);

/* ---- a genome-level screen by MinHash signatures ----------------------- */
/* What comes before mapping when a collection is larger than one index: which genomes are related at all.  Every genome is
 * reduced to a bottom-s MinHash signature of the minimizer hashes a sketch already holds in HBM, signatures are compared pair
 * by pair with Mash's merge rule, and the pairs above a Jaccard cut-off are grouped.
 *   1. Signature.  Genome g owns the records whose contig id lies in [sbf[g-1], sbf[g]) (sbf = sequencesByFileInfo, sbf[-1] =
 *      0); records are sorted by contig id.  With d_g the number of distinct hash values of g's records, the signature of g
 *      is the min(s, d_g) smallest of them, ascending as unsigned 32-bit; count[g] = min(s, d_g), 0 for a genome without
 *      records.  Layout: uint32 sig[n_genomes][s], int32 count[n_genomes]; entries from count[g] up to s are 0.  The count
 *      delimits a signature, not a sentinel: 0 and 0xFFFFFFFF are legal hashes.  1 <= s <= 4096.  This is the bottom-s
 *      sketch of the genome's winnowed minimizers, not of all its k-mers: a k-mer whose hash is among a contig's smallest
 *      is almost always some window's minimum, so the statistic is Mash-like at the sketch's k, not that of the Mash program.
 *   2. Pair statistic.  For signatures A and B made with the same s, U is their ascending distinct union, denom =
 *      min(s, |U|), shared = the number of the first denom elements of U that occur in both.  denom == 0 (two empty
 *      genomes) never forms a pair.
 *   3. Pair filter.  A pair is kept iff denom > 0 and (int64_t)shared * jd >= (int64_t)jn * denom: jn / jd is the
 *      caller's rational Jaccard cut-off, 0 <= jn <= jd, jd >= 1.  Integers only.
 *   4. Output.  Records sorted by (a, b); the same input gives the same bytes on every run.  Triangular: one set, the
 *      pairs a < b.  Rectangular: two sets, every (a, b), a indexing the first set and b the second.
 *   5. Groups.  The connected components of triangular records; labels[g] is the smallest genome number of g's group.
 * All three run like fa_table_best: on the calling thread's current device, on a stream of their own, with memory from the
 * device pool, finished when they return, FA_ERR_NO_DEVICE without a device. */
typedef struct fa_screen_pair {
  int32_t a, b;               /* triangular: a < b */
  int32_t shared, denom;      /* the Jaccard estimate is shared / denom */
} fa_screen_pair;             /* 16 bytes */
/* The genomes a workgroup of fa_screen_pairs takes per tile side at signature size s (a power of two, 2 .. 64); host only. */
int fa_screen_tile(int32_t s, int32_t *tile);
/* d_hash, d_seq_id (n_records each: the hash and contig id of every minimizer record), d_sig and d_count are DEVICE
 * pointers; sbf (n_genomes entries) is host memory.  FA_ERR_INVALID with nothing written: s outside [1, 4096]; d_seq_id not
 * ascending; a contig id outside [0, sbf[n_genomes-1]); sbf not non-decreasing. */
int fa_screen_signatures(const uint32_t *d_hash, const int32_t *d_seq_id, int64_t n_records, const int32_t *sbf, int32_t n_genomes,
                         int32_t s, uint32_t *d_sig, int32_t *d_count);
/* The signatures of the genomes [first, first + count) of a resident batch, made of the fragments the batch already holds:
 * queries are uploaded once, reduced to signatures, compared (fa_screen_pairs / fa_screen_contained /
 * fa_screen_contained_winner take the result as it is) and mapped.
 *   Signature.  That of genome g is taken from the query sketches of its fragments [genome_frag_lo[g], genome_frag_lo[g+1])
 *      -- the sets the mapper itself maps with, readable through fa_mapper_debug_query_sketch.  With d_g the number of
 *      distinct hashes in the union of those sketches, the signature is the min(s, d_g) smallest of them, ascending as
 *      unsigned 32-bit; count[g] = min(s, d_g); entries from count[g] up to s are 0.  A genome without fragments -- no
 *      contig, or only contigs shorter than a fragment -- has count 0.  Layout and the range 1 <= s <= 4096 are those of
 *      fa_screen_signatures.
 *   Relation to a sketch's signature.  A batch keeps only the whole fragments of each contig, and its windows do not cross
 *      fragment seams.  A genome's batch hash set is therefore a SUBSET of the hash set a sketch holds for the same contigs,
 *      and EQUALS that of a sketch to which every fragment was added as a contig of its own: the two signatures are close,
 *      not identical.
 *   Passes.  The fragments of the range are walked in order, in passes of at most pass_fragments fragments (0: the library's
 *      pass size, FA_PASS_FRAGMENTS), cut anywhere, not only at genome boundaries; a genome's partial signature is carried
 *      from pass to pass.  Memory beyond the mapper's workspace is bounded by the records of one pass.  The same input gives
 *      the same bytes on every run, for every pass_fragments.
 * d_sig ([count][s]) and d_count ([count]) are DEVICE pointers on the mapper's device; count == 0 is valid and writes
 * nothing.  stats may be NULL: [0] the fragments sketched, [1] the passes run (ceil(fragments / pass size), 0 for none), and,
 * only after fa_mapper_set_stage_events(m, 1), [2] the device time of the sketch kernel and [3] that of all passes, in
 * microseconds (0 otherwise).  FA_ERR_INVALID with nothing written: s out of range, a range outside the batch, a negative
 * pass_fragments, a NULL handle, NULL outputs with count > 0.  FA_ERR_NO_DEVICE without a device.  FA_ERR_UNSUPPORTED: a pass
 * whose tiles hold 2^31 record slots or more (two million tiles: only a pass_fragments far above the library's gets there).
 * The call is not a query.  It borrows a workspace of the mapper for the sketch kernel's staging arrays and runs on that
 * workspace's stream, finished when it returns; later queries give the rows they gave before, fa_mapper_last_timings and
 * fa_mapper_debug_spec still speak of the last query, and the stage getters (fa_mapper_debug_*) return what they returned
 * before the call: nothing they read is written here. */
int fa_genomes_signatures(fa_mapper *m, fa_genomes *g, int32_t first, int32_t count, int32_t s, int64_t pass_fragments,
                          uint32_t *d_sig, int32_t *d_count, int64_t *stats);
/* The signature arrays are DEVICE pointers; pairs_device != 0: `pairs` is one too.  triangular != 0 requires the same
 * pointers for both sets and n_a == n_b.  pairs == NULL only counts.  A `cap` below the number of pairs is FA_ERR_INVALID:
 * nothing is written, and *n_pairs holds the number needed.  FA_ERR_INVALID with nothing written, *n_pairs included: a count
 * outside [0, s]; a signature that does not ascend strictly below its count; s, jn or jd out of range.  n_pairs and stats
 * may be NULL; stats[0] the pairs evaluated, [1] the pairs kept. */
int fa_screen_pairs(const uint32_t *d_sig_a, const int32_t *d_count_a, int32_t n_a, const uint32_t *d_sig_b, const int32_t *d_count_b,
                    int32_t n_b, int32_t s, int triangular, int32_t jn, int32_t jd, fa_screen_pair *pairs, int64_t cap, int64_t *n_pairs,
                    int pairs_device, int64_t *stats);
/* labels [n_genomes] (a DEVICE pointer when labels_device != 0, as `pairs` is under pairs_device); *n_groups, which may be
 * NULL, is the number of g with labels[g] == g.  A record that is not 0 <= a < b < n_genomes is FA_ERR_INVALID and nothing
 * is written. */
int fa_screen_groups(const fa_screen_pair *pairs, int64_t n_pairs, int pairs_device, int32_t n_genomes, int32_t *labels, int labels_device,
                     int32_t *n_groups);

/* ---- the screen's containment road -------------------------------------- */
/* The Jaccard estimate of fa_screen_pairs collapses when two genomes differ in size: the bottom s of the union is filled by the
 * larger one, and a contig, a plasmid or an incomplete genome looks distant from the complete relative it lies inside.  The
 * containment of a query's signature in a reference's FULL set of distinct hashes (what `mash screen` computes) does not.
 *   1. Contents of a collection.  Genome g owns the records whose contig id lies in [sbf[g-1], sbf[g]), exactly as for
 *      signatures.  The contents are the distinct pairs (hash, genome) of the records, sorted ascending by hash as unsigned
 *      32-bit, then by genome.  Layout: uint32 ent_hash[m], int32 ent_genome[m]; m <= n_records; a genome without records has
 *      no entry; 0 and 0xFFFFFFFF are legal hashes.
 *   2. Statistic.  For a signature A (ascending, distinct, count_a long) and a reference genome b: shared = the number of
 *      elements x of A that have an entry (x, b); denom = count_a.  denom == 0 never forms a pair.
 *   3. Filter.  A pair is kept iff denom > 0 and (int64_t)shared * cd >= (int64_t)cn * denom: cn / cd is the caller's
 *      rational containment cut-off, 0 <= cn <= cd, cd >= 1.  Integers only.
 *   4. Output.  fa_screen_pair records sorted by (a, b), a indexing the signature set and b the collection; every pair is
 *      rectangular.  The same input gives the same bytes on every run.
 * Both calls run like fa_screen_pairs: on the calling thread's current device, on a stream of their own, with memory from the
 * device pool, finished when they return, FA_ERR_NO_DEVICE without a device. */
/* d_hash, d_seq_id, d_ent_hash and d_ent_genome are DEVICE pointers; sbf is host memory.  d_ent_hash == d_ent_genome == NULL
 * only counts.  A `cap` below the number of entries is FA_ERR_INVALID: nothing is written, and *n_entries (which may be NULL)
 * holds the number needed; n_records entries always suffice.  FA_ERR_INVALID with nothing written, *n_entries included:
 * d_seq_id not ascending; a contig id outside [0, sbf[n_genomes-1]); sbf not non-decreasing. */
int fa_screen_contents(const uint32_t *d_hash, const int32_t *d_seq_id, int64_t n_records, const int32_t *sbf, int32_t n_genomes,
                       uint32_t *d_ent_hash, int32_t *d_ent_genome, int64_t cap, int64_t *n_entries);
/* The references a workgroup of fa_screen_contained counts at a time: a collection of more is taken slice by slice; host only. */
int fa_screen_contain_slice(int32_t *slice);
/* The signature and entry arrays are DEVICE pointers; pairs_device != 0: `pairs` is one too.  pairs == NULL only counts.  A
 * `cap` below the number of pairs is FA_ERR_INVALID: nothing is written, and *n_pairs holds the number needed.
 * FA_ERR_INVALID with nothing written, *n_pairs included: s outside [1, 4096]; a count outside [0, s]; a signature that does
 * not ascend strictly below its count; entries that do not ascend strictly by (hash, genome); an entry's genome outside
 * [0, n_b); cn or cd out of range.  n_pairs and stats may be NULL; stats[0] the pairs evaluated, n_a * n_b, [1] the pairs
 * kept, [2] the directory entries visited: the entries (x, b) with x in A, summed over the signatures A. */
int fa_screen_contained(const uint32_t *d_sig, const int32_t *d_count, int32_t n_a, int32_t s, const uint32_t *d_ent_hash,
                        const int32_t *d_ent_genome, int64_t n_entries, int32_t n_b, int32_t cn, int32_t cd, fa_screen_pair *pairs,
                        int64_t cap, int64_t *n_pairs, int pairs_device, int64_t *stats);
/* Winner take all: fa_screen_contained with every element of a query credited to ONE reference, so that of a species'
 * many strains the one that explains the query best keeps its containment and the others fall to what they alone explain.
 * This is the library's integer restatement of `mash screen -w`, over the winnowed minimizers like everything here; it has
 * not been checked against the Mash program.  weight[b] >= 0 is per reference; d_weight == NULL: every weight is 0.
 *   1. First pass.  first[b] = the number of x in A with an entry (x, b): the `shared` of fa_screen_contained, over all the
 *      references of the collection.
 *   2. Winner.  For every x in A with at least one entry, winner(x) is the reference with the largest first[b] among those
 *      that have an entry (x, b) -- whether they pass the cut-off or not; ties go to the largest weight[b], remaining ties
 *      to the smallest b.  denom is the same for every b, so comparing first[] compares the identities exactly: integers only.
 *   3. Statistic.  won[b] = the number of x in A with winner(x) == b; denom = count_a.  The won[b] of a query sum to the
 *      number of its elements that occur anywhere in the collection.
 *   4. Filter and output.  Those of fa_screen_contained with `won` in the place of `shared`: kept iff denom > 0 and
 *      (int64_t)won * cd >= (int64_t)cn * denom, so cn == 0 keeps the references with won == 0; records {a, b, won, denom}
 *      sorted by (a, b); the same input gives the same bytes on every run.
 * Everything else is fa_screen_contained's contract: the pointers, counting only, a short `cap`, the causes of
 * FA_ERR_INVALID with nothing written -- and a negative weight is one more.  stats[0] is n_a * n_b, [1] the records kept,
 * [2] the directory entries visited by the first pass (the sum of first[], fa_screen_contained's [2]), [3] the elements
 * assigned (the sum of won[]): stats has four entries. */
int fa_screen_contained_winner(const uint32_t *d_sig, const int32_t *d_count, int32_t n_a, int32_t s, const uint32_t *d_ent_hash,
                               const int32_t *d_ent_genome, int64_t n_entries, int32_t n_b, const int32_t *d_weight, int32_t cn,
                               int32_t cd, fa_screen_pair *pairs, int64_t cap, int64_t *n_pairs, int pairs_device, int64_t *stats);
/* development: the threads of a workgroup of fa_screen_contained_winner's first kernel, 512 or 1024 (0: the default), for
 * the process; the results do not depend on it (scripts/time_contain_winner.py times both); host only */
int fa_debug_contain_winner_threads(int32_t threads);

/* stage-level introspection used by the parity tests */
int fa_mapper_debug_mappings(fa_mapper *m, fa_mapping *out, int64_t cap, int64_t *n); /* L2 results of the last query call, under its rules */
int fa_mapper_debug_l1(fa_mapper *m, int32_t *frag, int32_t *seq_id, int32_t *range_start, int32_t *range_end,
                       int64_t cap, int64_t *n);
int fa_mapper_debug_query_sketch(fa_mapper *m, int64_t fragment, uint32_t *hashes, int32_t cap, int32_t *sketch_size);
/* winnowed minimizers of one stand-alone sequence in query-fragment mode (seqId 0, fresh output vector) */
int fa_debug_sketch_sequence(const fa_params *params, const void *data, int64_t length, int char_width,
                             uint32_t *hash, int32_t *wpos, int64_t cap, int64_t *n);

/* development probe: workgroups of 128 threads with `lds_bytes` of dynamic LDS the chip holds at once */
int fa_debug_probe_occupancy(int lds_bytes, int *peak_alive);
/* raw bytes of the last call's event arena (the slide events) -- development aid */
int fa_mapper_debug_items(fa_mapper *m, void *out, int64_t bytes);
/* the query-independent slide geometry the index build derives per reference record: rec_prev,
 * rec_fwd, rec_bwd (4 bytes each) and the flag byte, `cap` records at most; *n = records of the index.  Checked against the
 * definitions by the parity tests (there is no counterpart in the reference: slidingMap.hpp keeps a std::map instead) */
int fa_mapper_debug_links(fa_mapper *m, int32_t *prev, int32_t *fwd, int32_t *bwd, uint8_t *flags, int64_t cap, int64_t *n);
/* slide events per L2 locus of the last call (two-kernel form), in locus order -- development aid */
int fa_mapper_debug_locus_events(fa_mapper *m, uint32_t *events, int64_t cap, int64_t *n);
/* last-call statistics: [0] sketch ms (K1 + fragment sort/unique), [1] lookup + L1 ms, [2] L2 ms, [3] CGI ms,
 * [4] total ms -- device time between stamps of the chip-wide 100 MHz counter that the first kernel of every stage
 * leaves in the pass's status block (the kernels of a pass run back to back on the library's stream) -- then counters
 * of the call: [5] reference records inside L2 locus ranges, [6] L2 loci, [7] L2 slide events, [8] loci redone with
 * the wide L2 state, [9] passes repeated because a speculated buffer size was too small; after fa_mapper_query also
 * the host-side wall-clock split of that call: [10] packing ms, [11] fragment / tile tables ms, [12] uploads ms,
 * [13] device pass + rows ms; [14], [15] development (fused L2 form); [16] the L2 stage once more, bracketed by HIP
 * events on the library's stream, when fa_mapper_set_stage_events is on (0 otherwise); [17] parts of the call whose sketch
 * stage ran as ONE launch (k_query_fused), [18] parts that ran K1 and the fragment sketch as two kernels, [19] parts whose
 * k_l2_events workgroups ran in the offset-major order; [23] positions per tile of the last fa_bench_sketch_kernel.  n <= 24. */
int fa_mapper_last_timings(fa_mapper *m, float *ms, int n);
/* The speculation record a mapper keeps across its calls, and the kernel forms of the last accepted part of the most
 * recently finished call: out[0 .. n) (entries beyond the 29 below are 0).  Reads only; takes the mapper lock.
 * Mapper-wide: [0] initialised, [1] smax (sketch bound of the LUTs and L2 tables), [2] seed_slots (LDS seed slots of k_l1,
 * follow the latest pass), [3] [4] [5] shares of the last accepted part's fragments in the small / middle / tiny size classes
 * of k_l1, in parts per million (-1 000 000: none seen yet), [6] l1_prefilter (sticky), [7] l1_no_small (sticky), [8] loci of
 * the last accepted part (l2_loci_last), [9] redo: the wide-state scan is launched (sticky), [10] fragments per part
 * (shrinks only), [11] fuse_skip, [12] fuse_penalty (back-off of k_query_fused), [13] smax_misses, [14] scratch words,
 * [15] slide-event capacity, [16] loci capacity.
 * Last part: [17] k_l1 launches (size classes), [18] [19] [20] their thread counts (0: none), [21] pre-filter on, [22] k_l2_scan
 * over sorted loci, [23] 32-bit slide events, [24] k_query_fused, [25] offset-major k_l2_events order, [26] wide-state scan
 * launched, [27] the sketch bound it ran with, [28] seed slots of its last k_l1 class.  A call that ran no part leaves 17-28 at 0.
 * Both layouts, this one and fa_mapper_last_timings', are generated from the tables of pyfastani_amd/csrc/fa_diag.h, which
 * names every entry; pyfastani_amd/diagnostics.py reads them by those names. */
int fa_mapper_debug_spec(fa_mapper *m, int64_t *out, int n);
/* on != 0: also bracket the L2 stage of every pass with two HIP events (slot [16] above).  Off by default: an event
 * record costs the stream about as much as a small kernel. */
int fa_mapper_set_stage_events(fa_mapper *m, int on);
/* the HIP stream the library launches on (so callers can bracket it with their own events) */
int fa_mapper_stream(fa_mapper *m, void **stream);
/* run only the minimizer-extraction kernel (K1) over a resident batch `repeat` times and report the mean
 * kernel time; used by bench.py for the roofline line.  The batch is sketched the way REFERENCE genomes are
 * (_fastani.pyx:651-659: whole contigs, windows across fragment boundaries): its fragments are joined into the contigs
 * they were cut from and tiled as fa_sketch tiles them. */
int fa_bench_sketch_kernel(fa_mapper *m, fa_genomes *g, int repeat, float *ms_per_launch, uint64_t *bases,
                           uint64_t *minimizers);

#ifdef __cplusplus
}
#endif
#endif /* FASTANI_HIP_H */
