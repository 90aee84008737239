// fa_ingest.h -- the contig bookkeeping of ingest: which contigs of a reference genome are sketched and what the genome's
// counters become (RefBook / RefStage), and which contigs of a query batch are mapped, how they are cut into fragments and
// where every part of the batch image lies (plan_batch).  Every rule restates a line of the reference's _fastani.pyx and is
// stated here once.  Plain C++ (no HIP): fa_engine.hip includes it for the library, scripts/host_sanitize.sh builds it with
// AddressSanitizer / UBSan on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "fa_error.h"

namespace fa {

// ----------------------------------------------------------------------------------------------------------
// reference side (Sketch.add_draft, _fastani.pyx:610-690)
// ----------------------------------------------------------------------------------------------------------
inline bool ref_admitted(const fa_params &P, int64_t length) { return length >= P.window_size && length >= P.kmer_size; }   // _fastani.pyx:648
inline uint64_t ref_counted(const fa_params &P, int64_t length) { return (uint64_t)(length / P.fragment_length) * P.fragment_length; }   // :680

// what a sketch knows of its genomes besides their sequence (skch::Sketch + pyfastani's counters)
struct RefBook {
  int64_t counter = 0;                    // contigs seen (Sketch._counter)
  uint64_t cur_total = 0;                 // counted length of the open genome (add_contig without end_genome so far)
  std::vector<uint64_t> lengths;          // per genome, rounded to whole fragments
  std::vector<int32_t> seqs_by_file;      // sequencesByFileInfo
  std::vector<int32_t> pending_contig;    // contig id of each admitted sequence that is not sketched yet
  void reset() { counter = 0; cur_total = 0; lengths.clear(); seqs_by_file.clear(); pending_contig.clear(); }
};

// what a call does with a genome that add_contig has left open (no end_genome yet)
enum class OpenGenome {
  FOLD,     // its contigs belong to the first genome the call closes (add_contig, end_genome, add_fasta)
  REFUSE,   // a call that brings whole genomes of its own fails (add_genomes, add_fasta_many, add_packed)
};

// Everything a call adds to a RefBook, built beside it: a refused contig, a missing file or an allocation failure in the
// packer leaves the book -- and with it the sketch -- exactly as it was (the reference keeps `total` in a local for the same
// reason, _fastani.pyx:618,680).
struct RefStage {
  int64_t counter;
  uint64_t cur_total;
  int64_t cur_short = 0;                  // contigs of the open genome that were not admitted
  std::vector<uint64_t> lengths;          // the genomes this call closes
  std::vector<int32_t> seqs_by_file;
  std::vector<int64_t> n_short;
  std::vector<int32_t> pending_contig;    // the contigs this call admits

  // `n_genomes`: how many genomes the call brings (a REFUSE call that brings none is allowed beside an open genome)
  RefStage(const RefBook &book, OpenGenome open, int64_t n_genomes = 1) : counter(book.counter), cur_total(book.cur_total) {
    FA_REQUIRE(open == OpenGenome::FOLD || book.cur_total == 0 || n_genomes == 0, FA_ERR_INVALID, "a genome is still open (add_contig without end_genome)");
  }
  // one contig of the open genome; true: it is sketched (the caller packs its sequence)
  bool contig(const fa_params &P, int64_t length) {
    FA_REQUIRE(length >= 0 && length < (1LL << 31), FA_ERR_INVALID, "contig length must be below 2^31");
    const bool admitted = ref_admitted(P, length);
    if (admitted) pending_contig.push_back((int32_t)counter); else cur_short++;
    cur_total += ref_counted(P, length);
    counter += 1;                                        // :683
    return admitted;
  }
  void end_genome() {
    lengths.push_back(cur_total);                        // :687
    seqs_by_file.push_back((int32_t)counter);            // :690
    n_short.push_back(cur_short);
    cur_total = 0; cur_short = 0;
  }
  // Contig c belongs to genome contig_genome[c] (non-decreasing; null: one genome) of the n_genomes the call brings, all
  // of which are closed.  admitted(c) for every contig that is sketched, in order.
  template <class Admitted>
  void genomes(const fa_params &P, const int64_t *len, const int32_t *contig_genome, int64_t n_contigs, int32_t n_genomes, Admitted admitted) {
    int32_t cur = 0;
    for (int64_t c = 0; c < n_contigs; c++) {
      const int32_t gi = contig_genome ? contig_genome[c] : 0;
      FA_REQUIRE(gi >= cur && gi < n_genomes, FA_ERR_INVALID, "contig_genome must be non-decreasing and < n_genomes");
      for (; cur < gi; cur++) end_genome();
      if (contig(P, len[c])) admitted(c);
    }
    for (; cur < n_genomes; cur++) end_genome();
  }
  // reserve, pack() (the one step that may still fail: it appends the admitted sequences to the store, all or nothing),
  // then insert -- nothing after the packer can throw
  template <class Pack>
  void commit(RefBook &book, Pack pack) {
    // (geometric: an exact reserve on every call would copy the whole list once per added contig)
    auto room = [](auto &v, size_t add) { if (v.size() + add > v.capacity()) v.reserve(std::max(v.size() + add, v.capacity() * 2)); };
    room(book.pending_contig, pending_contig.size());
    room(book.lengths, lengths.size());
    room(book.seqs_by_file, seqs_by_file.size());
    pack();
    book.pending_contig.insert(book.pending_contig.end(), pending_contig.begin(), pending_contig.end());
    book.lengths.insert(book.lengths.end(), lengths.begin(), lengths.end());
    book.seqs_by_file.insert(book.seqs_by_file.end(), seqs_by_file.begin(), seqs_by_file.end());
    book.counter = counter;
    book.cur_total = cur_total;
  }
  void commit(RefBook &book) { commit(book, [] {}); }
};

// ----------------------------------------------------------------------------------------------------------
// query side (Mapper._query_draft, _fastani.pyx:1061-1105): one batch of genomes, cut into fragments and tiles
// ----------------------------------------------------------------------------------------------------------
// Everything the kernels read of a batch sits in ONE device allocation, filled by ONE host-to-device copy from a staging
// image of the same layout: [packed 2-bit words | residue bytes | tiles | frag_tile_lo | frag_query | frag_qseq |
// total_frag], every part 16-byte aligned.
struct BatchLayout {
  struct Part { size_t at = 0, bytes = 0; };
  Part packed, bytes, tiles, frag_tile_lo, frag_query, frag_qseq, total_frag;
  size_t image_bytes = 0;
};

// a contig that holds fragments: contig `c` of the caller is sequence `si` of the packed store; its `nfrag` fragments are
// fragments nf0.. of the batch and q0.. of genome `gi`
struct ContigJob { int64_t c, si, nfrag, nf0, q0; int32_t gi; };

struct BatchPlan {
  std::vector<ContigJob> jobs;
  std::vector<int64_t> use_len;           // [jobs] bases of each that are packed: whole fragments (the tail is never read)
  std::vector<int64_t> genome_frag_lo;    // [n_genomes + 1] fragment range of each genome
  std::vector<int64_t> contig_frag_lo;    // [jobs] first fragment of each (ascending)
  std::vector<uint64_t> total_fragments, total_length;
  std::vector<int32_t> n_short;
  uint64_t total_bases = 0;               // bases inside fragments
  int64_t F = 0, tiles_per_frag = 0, ntiles = 0;
  size_t bases = 0;                       // of the store: every packed contig padded to 64
  BatchLayout at;
};

// `tile_positions`: k-mer positions per tile; `tile_bytes`: size of a tile descriptor (both of the sketch kernel)
inline BatchPlan plan_batch(const fa_params &P, const int64_t *lengths, const int32_t *contig_genome, int64_t n_contigs, int32_t n_genomes,
                            int tile_positions, size_t tile_bytes) {
  BatchPlan b;
  const int frag = P.fragment_length;
  const int64_t min_len = std::min<int64_t>(std::min(P.window_size, P.kmer_size), frag);
  b.genome_frag_lo.assign((size_t)n_genomes + 1, 0);
  b.total_fragments.assign((size_t)n_genomes, 0); b.total_length.assign((size_t)n_genomes, 0); b.n_short.assign((size_t)n_genomes, 0);
  int32_t cur = 0;
  for (int64_t c = 0; c < n_contigs; c++) {
    const int32_t gi = contig_genome ? contig_genome[c] : 0;
    FA_REQUIRE(gi >= cur && gi < n_genomes, FA_ERR_INVALID, "contig_genome must be non-decreasing and < n_genomes");
    while (cur < gi) { cur++; b.genome_frag_lo[(size_t)cur] = b.F; }
    const int64_t len = lengths[c];
    if (len < min_len) { b.n_short[(size_t)gi]++; continue; }          // _fastani.pyx:1061-1070
    const int64_t nfrag = len / frag;                                   // :1097
    if (nfrag > 0) {                                                    // querySeqId = fragments before + i, :985
      b.jobs.push_back(ContigJob{c, (int64_t)b.jobs.size(), nfrag, b.F, (int64_t)b.total_fragments[(size_t)gi], gi});
      b.use_len.push_back(nfrag * frag);
      b.contig_frag_lo.push_back(b.F);
      b.bases += (size_t)((nfrag * frag + 63) / 64 * 64);
      b.F += nfrag;
    }
    b.total_fragments[(size_t)gi] += (uint64_t)nfrag;                   // :1104
    b.total_length[(size_t)gi] += (uint64_t)len;                        // :1105
    b.total_bases += (uint64_t)(nfrag * frag);
  }
  while (cur < n_genomes) { cur++; b.genome_frag_lo[(size_t)cur] = b.F; }
  const int64_t npos_frag = (int64_t)frag - P.kmer_size + 1;
  b.tiles_per_frag = npos_frag > 0 ? (npos_frag + tile_positions - 1) / tile_positions : 0;
  b.ntiles = b.F * b.tiles_per_frag;
  FA_REQUIRE(b.ntiles < (1LL << 31) - 1 && b.F < (1LL << 31) - 1, FA_ERR_UNSUPPORTED, "too many fragments in one batch");
  const bool protein = P.alphabet_size != 4;
  size_t end = 0;
  auto part = [&](size_t bytes) { BatchLayout::Part p; p.at = end; p.bytes = (bytes + 15) / 16 * 16; end += p.bytes; return p; };
  b.at.packed = part(protein ? 0 : b.bases / 4 + 64);                   // (the slack: the sketch kernel's funnel shift reads one word past the end)
  b.at.bytes = part(protein ? b.bases + 64 : 0);
  b.at.tiles = part((size_t)std::max<int64_t>(b.ntiles, 1) * tile_bytes);
  b.at.frag_tile_lo = part(((size_t)b.F + 1) * 4);
  b.at.frag_query = part((size_t)std::max<int64_t>(b.F, 1) * 4);
  b.at.frag_qseq = part((size_t)std::max<int64_t>(b.F, 1) * 4);
  b.at.total_frag = part((size_t)std::max(n_genomes, 1) * 4);
  b.at.image_bytes = end;
  return b;
}

}  // namespace fa
