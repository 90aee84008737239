// Host-side pieces of libfastani_hip under AddressSanitizer + UBSan, and (separately) ThreadSanitizer, on the CPU:
//   the 2-bit packer (fa_host.h: AVX2 path, scalar exception path, wide characters, protein bytes) on the persistent thread
//   pool, the memory-mapped FASTA reader (fa_fasta.h), the statistics tables (fa_stats.h), the workspace lease and the
//   pinned-word spin (fa_lease.h), the policy of a query pass (fa_policy.h: every rule at the boundaries where it turns), the contig bookkeeping of
//   ingest (fa_ingest.h: the reference roads and the plan of a query batch against restatements of _fastani.pyx).  Inputs: the edge cases of tests/test_gpu_parity.py::test_minimizer_streams and
//   tests/test_fasta.py, plus four concurrent clients.  No HIP: these headers are what the library's one translation unit (fa_engine.hip and the fa_*.hip.h it includes) uses for the same jobs.
// Built and run by scripts/host_sanitize.sh; exits non-zero on any mismatch (the sanitizers abort on their own findings).
#include <unistd.h>

#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../pyfastani_amd/csrc/fa_fasta.h"
#include "../../pyfastani_amd/csrc/fa_host.h"
#include "../../pyfastani_amd/csrc/fa_ingest.h"
#include "../../pyfastani_amd/csrc/fa_lease.h"
#include "../../pyfastani_amd/csrc/fa_policy.h"
#include "../../pyfastani_amd/csrc/fa_stats.h"

using namespace fa;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// ---- reference packer: the definition of the store, byte by byte ----
struct Plain { std::vector<uint32_t> packed; std::vector<uint8_t> bytes; std::vector<int64_t> epos; std::vector<uint8_t> eval; std::vector<int64_t> off; int64_t total = 0; };
static uint8_t up(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c; }
static void plain_append(Plain &p, bool protein, const std::vector<uint32_t> &seq) {   // seq as code points (any width)
  const int64_t len = (int64_t)seq.size(), padded = (len + 63) / 64 * 64;
  p.off.push_back(p.total);
  if (protein) {
    for (int64_t i = 0; i < padded; i++) p.bytes.push_back(i < len ? up((uint8_t)seq[i]) : 0);
  } else {
    const size_t w0 = p.packed.size();
    p.packed.resize(w0 + padded / 16, 0u);
    for (int64_t i = 0; i < len; i++) {
      const uint8_t c = up((uint8_t)seq[i]);
      int code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
      if (code < 0) { p.epos.push_back(p.total + i); p.eval.push_back(c); code = 0; }
      p.packed[w0 + i / 16] |= (uint32_t)code << (2 * (i % 16));
    }
  }
  p.total += padded;
}

template <class A, class B> static bool same_vec(const A &a, const B &b) { return a.size() == b.size() && std::equal(a.begin(), a.end(), b.begin()); }
template <class T> static std::vector<T> widen(const std::vector<uint32_t> &s) { return std::vector<T>(s.begin(), s.end()); }

static std::vector<std::vector<uint32_t>> edge_sequences(std::mt19937_64 &rng) {
  auto str = [](const std::string &s) { return std::vector<uint32_t>(s.begin(), s.end()); };
  std::vector<std::vector<uint32_t>> v;
  v.push_back({});
  v.push_back(str("A"));
  v.push_back(str("ACGTACGTACGTACG"));                       // 15: one partial word
  v.push_back(str("ACGTACGTACGTACGT"));                      // 16
  v.push_back(str("acgtacgtacgtacgtN"));                     // lower case + an exception in the tail word
  v.push_back(str(std::string(31, 'T') + "N" + std::string(33, 'g')));
  v.push_back(str(std::string(200, 'N')));                   // exceptions only
  v.push_back(str("ACGTRYKMSWBDHVNacgtrykmswbdhvn*-." + std::string(70, 'C')));   // IUPAC, both cases, punctuation
  const char alpha[] = "ACGTacgtNnRYKM";
  for (int len : {17, 63, 64, 65, 127, 128, 1000, 4097, 70001, 300017}) {
    std::vector<uint32_t> s((size_t)len);
    const int exc_every = len > 5000 ? 3001 : 37;            // long runs of plain bases (the AVX2 path) with rare exceptions
    for (int i = 0; i < len; i++) s[(size_t)i] = (i % exc_every == exc_every - 1) ? (uint32_t)alpha[8 + rng() % 6] : (uint32_t)alpha[rng() % 8];
    v.push_back(std::move(s));
  }
  return v;
}

static void test_packer(bool protein, int width, int clients) {
  std::mt19937_64 rng(1234 + width + (protein ? 100 : 0));
  const auto seqs = edge_sequences(rng);
  auto one_client = [&](int id) {
    HostStore hs; hs.protein = protein;
    Plain want;
    // contig by contig, then several at once (append_many), as Sketch.add_draft and upload_genomes do
    std::vector<std::vector<uint8_t>> s8; std::vector<std::vector<uint16_t>> s16; std::vector<std::vector<uint32_t>> s32;
    std::vector<const void *> ptrs; std::vector<int64_t> lens;
    for (auto &s : seqs) {
      if (width == 1) { s8.push_back(widen<uint8_t>(s)); ptrs.push_back(s8.back().data()); }
      else if (width == 2) { s16.push_back(widen<uint16_t>(s)); ptrs.push_back(s16.back().data()); }
      else { s32.push_back(s); ptrs.push_back(s32.back().data()); }
      lens.push_back((int64_t)s.size());
    }
    for (size_t i = 0; i < seqs.size() / 2; i++) { hs.append(ptrs[i], width, lens[i]); plain_append(want, protein, seqs[i]); }
    const size_t rest = seqs.size() - seqs.size() / 2;
    hs.append_many(ptrs.data() + seqs.size() / 2, lens.data() + seqs.size() / 2, (int64_t)rest, width);
    for (size_t i = seqs.size() / 2; i < seqs.size(); i++) plain_append(want, protein, seqs[i]);
    CHECK(hs.total == want.total, "client %d: store length %lld vs %lld", id, (long long)hs.total, (long long)want.total);
    CHECK(hs.seq_off == want.off, "client %d: sequence offsets differ", id);
    if (protein) CHECK(same_vec(hs.bytes, want.bytes), "client %d: protein bytes differ", id);
    else {
      CHECK(same_vec(hs.packed, want.packed), "client %d: packed words differ (width %d)", id, width);
      CHECK(hs.exc_pos == want.epos && hs.exc_val == want.eval, "client %d: exception lists differ (%zu vs %zu)", id, hs.exc_pos.size(), want.epos.size());
    }
    // pack_many into caller memory that is exactly as large as promised (ASan guards its ends)
    HostStore h2; h2.protein = protein;
    const int64_t add = HostStore::padded_bases(lens.data(), (int64_t)lens.size());
    std::vector<uint32_t> d32(protein ? 0 : (size_t)add / 16);
    std::vector<uint8_t> d8(protein ? (size_t)add : 0);
    h2.pack_many(ptrs.data(), lens.data(), (int64_t)lens.size(), width, protein ? nullptr : d32.data(), protein ? d8.data() : nullptr);
    if (protein) CHECK(d8 == want.bytes, "client %d: pack_many bytes differ", id); else CHECK(d32 == want.packed, "client %d: pack_many words differ", id);
  };
  std::vector<std::thread> th;
  for (int c = 0; c < clients; c++) th.emplace_back(one_client, c);
  for (auto &t : th) t.join();
}

static std::string write_tmp(const std::string &name, const std::string &content) {
  char dir[] = "/tmp/fa_sanitize_XXXXXX";
  static std::string base = mkdtemp(dir);
  const std::string path = base + "/" + name;
  FILE *f = fopen(path.c_str(), "wb");
  fwrite(content.data(), 1, content.size(), f);
  fclose(f);
  return path;
}

static void test_fasta(int clients) {
  struct Case { std::string name, text; std::vector<std::pair<std::string, std::string>> want; bool buffer_error; };
  std::string big;                                              // one record of > 256 KiB: cut into pieces at line starts
  std::string big_seq;
  for (int i = 0; i < 9000; i++) { std::string line(60, "acgtn"[i % 5]); big += line + "\n"; for (char c : line) big_seq += (char)up((uint8_t)c); }
  std::vector<Case> cases = {
    {"empty.fa", "", {}, false},
    {"noheader.fa", "ACGT\n>x\nAC\n", {}, false},                // first line is not a header: no records at all
    {"one.fa", ">id one\nACgt\nNNac\n", {{"id one", "ACGTNNAC"}}, false},
    {"noeol.fa", ">a\nAC\n>b\nGT", {{"a", "AC"}, {"b", "GT"}}, false},
    {"emptyrec.fa", ">a\n>b\n\nAC\n\n>c\n", {{"a", ""}, {"b", "AC"}, {"c", ""}}, false},
    {"gt_inside.fa", ">a\nAC>GT\nTT\n", {{"a", "AC>GTTT"}}, false}, // '>' that is not at a line start belongs to the body
    {"big.fa", ">big\n" + big + ">tail\nAC\n", {{"big", big_seq}, {"tail", "AC"}}, false},
    {"longid.fa", ">" + std::string(3000, 'x') + "\nAC\n", {}, true},
    {"headeronly_noeol.fa", ">abc", {}, true},                   // the reference insists on the newline
  };
  auto one_client = [&](int id) {
    for (auto &c : cases) {
      const std::string path = write_tmp(std::to_string(id) + "_" + c.name, c.text);
      bool threw = false;
      std::vector<std::pair<std::string, std::string>> got;
      try {
        FastaFile f; f.open(path.c_str());
        while (f.next()) got.emplace_back(f.id, std::string(f.seq.begin(), f.seq.end()));
      } catch (const Error &e) { threw = e.code == FA_ERR_BUFFER; }
      CHECK(threw == c.buffer_error, "%s: buffer error %d, expected %d", c.name.c_str(), (int)threw, (int)c.buffer_error);
      if (!c.buffer_error) CHECK(got == c.want, "%s: records differ (%zu vs %zu)", c.name.c_str(), got.size(), c.want.size());
      threw = false;
      std::vector<FastaSeq> seqs;
      try { read_fasta_records(path.c_str(), seqs); } catch (const Error &e) { threw = e.code == FA_ERR_BUFFER; }
      CHECK(threw == c.buffer_error, "%s (bulk): buffer error %d, expected %d", c.name.c_str(), (int)threw, (int)c.buffer_error);
      if (!c.buffer_error) {
        CHECK(seqs.size() == c.want.size(), "%s (bulk): %zu records vs %zu", c.name.c_str(), seqs.size(), c.want.size());
        for (size_t r = 0; r < seqs.size() && r < c.want.size(); r++)
          CHECK(std::string((const char *)seqs[r].data.get(), seqs[r].size) == c.want[r].second, "%s (bulk): record %zu differs", c.name.c_str(), r);
      }
      unlink(path.c_str());
    }
    bool io = false;
    try { FastaFile f; f.open("/nonexistent/fa.fa"); } catch (const Error &e) { io = e.code == FA_ERR_IO; }
    CHECK(io, "a missing file should fail with FA_ERR_IO");
    io = false;
    try { FastaFile f; f.open("/tmp"); } catch (const Error &e) { io = e.code == FA_ERR_IO; }
    CHECK(io, "a directory should fail with FA_ERR_IO");
  };
  std::vector<std::thread> th;
  for (int c = 0; c < clients; c++) th.emplace_back(one_client, c);
  for (auto &t : th) t.join();
}

// read_fasta_packed (one sweep from file bytes to 2-bit words) and place_packed against the definition: the records of
// FastaFile, packed byte by byte; whole records and prefixes (a query batch holds whole fragments only); many files at once
static void test_fasta_packed(bool protein) {
  std::mt19937_64 rng(protein ? 77 : 78);
  std::vector<std::string> texts = {
    "", "ACGT\n>x\nAC\n", ">id one\nACgt\nNNac\n", ">a\nAC\n>b\nGT", ">a\n>b\n\nAC\n\n>c\n", ">a\nAC>GT\nTT\n", ">crlf\r\nACGT\r\nAC\r\n",
    ">x\n" + std::string(31, 'A') + "\n" + std::string(32, 'C') + "\n" + std::string(33, 'G') + "\n" + std::string(64, 'T') + "\n" + std::string(65, 'a') + "\nN",
  };
  const char alpha[] = "ACGTACGTACGTACGTacgtNnRYKM*";
  for (int t = 0; t < 40; t++) {                                   // random files: 1-6 records, line widths 1-100, rare exceptions
    std::string text;
    const int nrec = 1 + (int)(rng() % 6);
    for (int r = 0; r < nrec; r++) {
      text += ">rec" + std::to_string(r) + " some description\n";
      const size_t len = (rng() % 5 == 0) ? rng() % 70 : rng() % 20000;
      const size_t width = 1 + rng() % 100;
      const bool dirty = rng() % 3 == 0;
      for (size_t i = 0; i < len; i++) {
        text += dirty && rng() % 50 == 0 ? alpha[rng() % (sizeof(alpha) - 1)] : "ACGT"[rng() % 4];
        if ((i + 1) % width == 0) text += '\n';
      }
      if (rng() % 4) text += '\n';
      if (rng() % 8 == 0) text += "\n\n";
    }
    texts.push_back(text);
  }
  std::vector<std::string> paths;
  for (size_t i = 0; i < texts.size(); i++) paths.push_back(write_tmp("packed_" + std::to_string(i) + ".fa", texts[i]));
  std::vector<const char *> cpaths;
  for (auto &p : paths) cpaths.push_back(p.c_str());
  std::vector<PackedFasta> files;
  read_fasta_packed_many(cpaths.data(), cpaths.size(), protein, files);
  HostStore whole, part;
  whole.protein = part.protein = protein;
  Plain want_whole, want_part;
  std::vector<PackedRef> refs_whole, refs_part;
  for (size_t i = 0; i < texts.size(); i++) {
    FastaFile f; f.open(paths[i].c_str());
    size_t r = 0;
    while (f.next()) {
      CHECK(r < files[i].rec_len.size() && files[i].rec_len[r] == (int64_t)f.seq.size(), "file %zu record %zu: %lld bases vs %zu", i, r,
            r < files[i].rec_len.size() ? (long long)files[i].rec_len[r] : -1LL, f.seq.size());
      if (r >= files[i].rec_len.size()) break;
      std::vector<uint32_t> seq(f.seq.begin(), f.seq.end());
      plain_append(want_whole, protein, seq);
      refs_whole.push_back(PackedRef{&files[i], (int64_t)r, (int64_t)seq.size()});
      const int64_t cut = seq.empty() ? 0 : (int64_t)(rng() % (seq.size() + 1));
      seq.resize((size_t)cut);
      plain_append(want_part, protein, seq);
      refs_part.push_back(PackedRef{&files[i], (int64_t)r, cut});
      r++;
    }
    CHECK(r == files[i].rec_len.size(), "file %zu: %zu records vs %zu", i, files[i].rec_len.size(), r);
  }
  append_packed(whole, refs_whole.data(), (int64_t)refs_whole.size());
  append_packed(part, refs_part.data(), (int64_t)refs_part.size());
  auto same = [&](const HostStore &hs, const Plain &w, const char *what) {
    CHECK(hs.total == w.total, "%s: total %lld vs %lld", what, (long long)hs.total, (long long)w.total);
    CHECK(hs.seq_off == w.off, "%s: sequence offsets differ", what);
    if (protein) CHECK(same_vec(hs.bytes, w.bytes), "%s: bytes differ", what); else CHECK(same_vec(hs.packed, w.packed), "%s: packed words differ", what);
    CHECK(hs.exc_pos == w.epos && hs.exc_val == w.eval, "%s: exceptions differ (%zu vs %zu)", what, hs.exc_pos.size(), w.epos.size());
  };
  same(whole, want_whole, protein ? "packed fasta, protein, whole records" : "packed fasta, whole records");
  same(part, want_part, protein ? "packed fasta, protein, prefixes" : "packed fasta, prefixes");
  bool threw = false;
  const std::string longid = write_tmp("packed_longid.fa", ">" + std::string(3000, 'x') + "\nAC\n");
  try { PackedFasta pf; read_fasta_packed(longid.c_str(), protein, pf); } catch (const Error &e) { threw = e.code == FA_ERR_BUFFER; }
  CHECK(threw, "over-long identifier should fail with FA_ERR_BUFFER in the packed reader");
  threw = false;
  const char *missing[2] = {paths[2].c_str(), "/nonexistent/fa.fa"};
  try { std::vector<PackedFasta> v; read_fasta_packed_many(missing, 2, protein, v); } catch (const Error &e) { threw = e.code == FA_ERR_IO; }
  CHECK(threw, "a missing file among many should fail with FA_ERR_IO");
  unlink(longid.c_str());
  for (auto &p : paths) unlink(p.c_str());
}

static void test_stats() {
  CHECK(stat_recommended_window(1e-3, 16, 4, 80.0f, 3000, 5000000ULL) == 24, "default window is 24 (test_ani.py:60)");
  StatTables t; t.k = 16; t.pid = 80.0f; t.smax = -1;
  CHECK(t.extend(64), "tables grow");
  CHECK(!t.extend(32), "tables never shrink");
  CHECK(t.extend(300), "tables grow again");
  CHECK((int)t.min_hits.size() >= 301 && (int)t.pass_shared.size() >= 301, "table sizes");
  for (int s = 1; s <= 300; s += 13) {
    CHECK(t.min_hits[(size_t)s] == stat_min_hits_relaxed(s, 16, 80.0f), "minHits[%d]", s);
    float id = 0, upper = 0;
    stat_identity(s / 2, s, 16, &id, &upper);
    CHECK(id >= 0.0f && id <= 100.0f && upper >= id, "identity(%d, %d) = %f <= %f", s / 2, s, id, upper);
  }
  for (int k : {3, 5, 14, 16, 21}) for (int s : {1, 2, 17, 263}) { (void)stat_min_hits_relaxed(s, k, 80.0f); (void)stat_min_hits_relaxed(s, k, 99.9f); }
}

struct FakeWs { bool in_use = false; int prepared = 0; std::atomic<int> users{0}; };
struct FakeOwner { static constexpr int NWS = 4; std::mutex mtx; std::condition_variable ws_free; FakeWs ws[NWS]; int last_ws = 0; };

static void test_lease(int threads) {
  FakeOwner m;
  std::atomic<int> thrown{0}, served{0};
  auto client = [&](int id) {
    for (int it = 0; it < 400; it++) {
      try {
        Lease<FakeOwner, FakeWs> l(m, [&](FakeWs &w) { if ((id + it) % 37 == 0) throw Error(FA_ERR_NO_DEVICE, "stream"); w.prepared++; });
        CHECK(l.w->users.fetch_add(1) == 0, "two calls on one workspace");
        if (it % 16 == 0) std::this_thread::yield();
        l.w->users.fetch_sub(1);
        served++;
      } catch (const Error &) { thrown++; }
    }
  };
  std::vector<std::thread> th;
  for (int c = 0; c < threads; c++) th.emplace_back(client, c);
  for (auto &t : th) t.join();
  CHECK(served + thrown == threads * 400 && thrown > 0, "every call either ran or failed in prepare (%d + %d)", served.load(), thrown.load());
  for (auto &w : m.ws) CHECK(!w.in_use, "a workspace was not handed back");
}

static void test_spin() {
  alignas(64) uint32_t word = 0;
  uint32_t payload = 0;
  std::thread pub([&] { std::this_thread::sleep_for(std::chrono::milliseconds(3)); payload = 77; __atomic_store_n(&word, 5u, __ATOMIC_RELEASE); });
  const bool ok = spin_for_seq(&word, 5u, 2000000);
  CHECK(ok && payload == 77, "the released word and what was written before it");
  pub.join();
  CHECK(!spin_for_seq(&word, 6u, 200), "a word that never comes times out");
  CHECK(!spin_for_seq(&word, 6u, 0) && spin_for_seq(&word, 5u, 0), "no spinning: one look");
}


// ---- the policy of a query pass (fa_policy.h) ----
static Spec fresh_spec() { return spec_first_use(256, 1 << 18, 1ULL << 26, 48 * 1024); }
static PassStatus quiet_status() { PassStatus s; memset(&s, 0, sizeof s); return s; }
static Forms ran_with(bool prefilter, int n_l1, int first_nt) {
  Forms f; f.prefilter = prefilter; f.n_l1 = n_l1;
  for (int c = 0; c < n_l1; c++) f.l1_threads[c] = c == 0 ? first_nt : 512;
  return f;
}
// the verdict on a part of F fragments with one locus region of 1 024, events up to 2^32
static Verdict verdict(Spec &sp, const PassStatus &s, int64_t F = 1000, const Forms &ran = Forms(), uint64_t items_max = 1ULL << 32,
                       int (*occ)(int) = [](int) { return 0; }, uint32_t loci_n = 1, uint32_t loci_shift = 10) {
  return judge(sp, s, ran, F, loci_n, loci_shift, items_max, occ);
}

static void test_policy_sketch_bound() {
  // first growth: the tight multiple of 8 (the smallest one >= largest sketch + 4)
  for (int seen : {257, 260, 261, 268, 269, 276, 277}) {
    Spec sp = fresh_spec();
    PassStatus s = quiet_status(); s.stats[STAT_SMAX] = seen; s.pinfo[PI_FLAGS] = SPEC_SMAX;
    const Verdict v = verdict(sp, s);
    const int want = seen <= 260 ? 264 : seen <= 268 ? 272 : seen <= 276 ? 280 : 288;
    CHECK(sp.smax == want && sp.smax_misses == 1, "tight bound for %d: %d (want %d)", seen, sp.smax, want);
    CHECK(v.kind == Verdict::VOIDED && v.miss, "a sketch above the bound voids the part");
  }
  {  // no growth at the bound itself
    Spec sp = fresh_spec(); PassStatus s = quiet_status(); s.stats[STAT_SMAX] = 256;
    verdict(sp, s);
    CHECK(sp.smax == 256 && sp.smax_misses == 0, "a sketch at the bound keeps it");
  }
  // later growths: the largest bound up to the roomy one (an eighth of headroom) that keeps the tight bound's occupancy
  Spec sp = fresh_spec(); sp.smax_misses = 1;
  PassStatus s = quiet_status(); s.stats[STAT_SMAX] = 400; s.pinfo[PI_FLAGS] = SPEC_SMAX;   // tight 408, roomy 456
  verdict(sp, s, 1000, Forms(), 1ULL << 32, [](int b) { return b <= 432 ? 9 * 64 + 6 : 8 * 64 + 6; });
  CHECK(sp.smax == 432 && sp.smax_misses == 2, "roomy bound kept to the occupancy of the tight one: %d", sp.smax);
  sp = fresh_spec(); sp.smax_misses = 1;
  verdict(sp, s, 1000, Forms(), 1ULL << 32, [](int) { return 7; });
  CHECK(sp.smax == 456, "the same occupancy all the way: the roomy bound, %d", sp.smax);
  sp = fresh_spec(); sp.smax_misses = 1;
  verdict(sp, s, 1000, Forms(), 1ULL << 32, [](int b) { return b == 408 ? 7 : 6; });
  CHECK(sp.smax == 408, "occupancy drops above the tight bound: %d", sp.smax);
  sp = fresh_spec(); sp.smax_misses = 1;
  verdict(sp, s);
  CHECK(sp.smax == 456, "occupancy unknown: the roomy bound, %d", sp.smax);
}

static void test_policy_seed_slots() {
  const struct { uint64_t max_seeds; uint32_t want; } cases[] = {
    {0, 1024}, {819, 1024}, {820, 1280}, {4000, 5120}, {4096, 5120}, {1ULL << 40, lds_seed_cap_max(256)}};
  for (auto c : cases) {
    Spec sp = fresh_spec(); PassStatus s = quiet_status(); s.totals[TOT_MAX_FRAG] = c.max_seeds;
    const Verdict v = verdict(sp, s);
    CHECK(v.kind == Verdict::ACCEPTED && sp.seed_slots == c.want, "seed slots for %llu hits: %u (want %u)", (unsigned long long)c.max_seeds, sp.seed_slots, c.want);
  }
  CHECK(lds_seed_cap_max(256) == 36864 && lds_seed_cap_max(2000) == 35584 && lds_seed_cap_max(1 << 30) == 256, "lds_seed_cap_max");
  // a void part adopts the new slots only together with SPEC_SCRATCH
  Spec sp = fresh_spec(); PassStatus s = quiet_status(); s.totals[TOT_MAX_FRAG] = 100; s.pinfo[PI_FLAGS] = SPEC_LOCI;
  verdict(sp, s);
  CHECK(sp.seed_slots == 4096, "void without SPEC_SCRATCH keeps the slots: %u", sp.seed_slots);
  sp = fresh_spec(); s.pinfo[PI_FLAGS] = SPEC_SCRATCH; s.totals[TOT_SCRATCH] = 1000;
  verdict(sp, s);
  CHECK(sp.seed_slots == 1024 && sp.scratch_words == 1250, "void with SPEC_SCRATCH adopts the slots (%u) and a quarter of headroom (%llu)", sp.seed_slots,
        (unsigned long long)sp.scratch_words);
}

static void test_policy_loci_events_seeds() {
  {  // doubling
    Spec sp = fresh_spec(); PassStatus s = quiet_status(); s.pinfo[PI_FLAGS] = SPEC_LOCI; s.loci_region[0] = 1100;
    CHECK(verdict(sp, s).kind == Verdict::VOIDED && sp.l_cap == 2 << 18, "loci: the capacity doubles (%lld)", (long long)sp.l_cap);
  }
  {  // sized for the fullest region
    Spec sp = fresh_spec(); sp.l_cap = 1000; PassStatus s = quiet_status(); s.pinfo[PI_FLAGS] = SPEC_LOCI;
    s.loci_region[0] = 100; s.loci_region[1] = 3000; s.loci_region[2] = 50;
    verdict(sp, s, 1000, Forms(), 1ULL << 32, [](int) { return 0; }, 4, 8);
    CHECK(sp.l_cap == 24000, "loci: twice the fullest region times the regions (%lld)", (long long)sp.l_cap);
  }
  const int64_t l_max = (1LL << 31) - 64, at_cap = 1LL << 24;   // 64 regions at the cap hold 2^24 loci each
  {  // the fullest region fits at the cap: grow to it
    Spec sp = fresh_spec(); sp.l_cap = 1LL << 30; PassStatus s = quiet_status(); s.pinfo[PI_FLAGS] = SPEC_LOCI; s.loci_region[5] = (uint32_t)at_cap;
    const Verdict v = verdict(sp, s, 1000, Forms(), 1ULL << 32, [](int) { return 0; }, 64, 20);
    CHECK(v.kind == Verdict::VOIDED && sp.l_cap == l_max && sp.part_frags == 48 * 1024, "loci: up to the cap (%lld)", (long long)sp.l_cap);
  }
  {  // it does not: the part shrinks
    Spec sp = fresh_spec(); sp.l_cap = 1LL << 30; PassStatus s = quiet_status(); s.pinfo[PI_FLAGS] = SPEC_LOCI; s.loci_region[5] = (uint32_t)at_cap + 1;
    const Verdict v = verdict(sp, s, 1000, Forms(), 1ULL << 32, [](int) { return 0; }, 64, 20);
    CHECK(v.kind == Verdict::SHRUNK && sp.part_frags == 500 && sp.l_cap == 1LL << 30, "loci: a region the cap cannot hold shrinks the part (%lld)", (long long)sp.part_frags);
    sp = fresh_spec(); sp.l_cap = 1LL << 30;
    CHECK(verdict(sp, s, 1, Forms(), 1ULL << 32, [](int) { return 0; }, 64, 20).kind == Verdict::FAILED, "loci: one fragment cannot shrink");
  }
  {  // events: the arena grows for the fullest region, by half again at least twice
    Spec sp = fresh_spec(); PassStatus s = quiet_status(); s.pinfo[PI_FLAGS] = SPEC_EVENTS; s.ev_region[3] = 1000;
    verdict(sp, s, 100);                                         // 8 regions: 8 000 events needed
    CHECK(sp.items_cap == 1ULL << 27, "events: doubling (%llu)", (unsigned long long)sp.items_cap);
    sp = fresh_spec(); sp.items_cap = 1000;
    verdict(sp, s, 100);
    CHECK(sp.items_cap == 10000, "events: the need and a quarter (%llu)", (unsigned long long)sp.items_cap);
    sp = fresh_spec(); sp.items_cap = 1000; s.pinfo[PI_EVENTS] = 20000;
    verdict(sp, s, 100, Forms(), 30000);
    CHECK(sp.items_cap == 25000, "events: the fused form's counter (%llu)", (unsigned long long)sp.items_cap);
    sp = fresh_spec(); sp.items_cap = 1000;
    verdict(sp, s, 100, Forms(), 24000);
    CHECK(sp.items_cap == 24000, "events: at most items_max (%llu)", (unsigned long long)sp.items_cap);
    sp = fresh_spec(); s.pinfo[PI_EVENTS] = 0;
    const Verdict v = verdict(sp, s, 100, Forms(), 7999);
    CHECK(v.kind == Verdict::SHRUNK && sp.part_frags == 50, "events: beyond items_max the part shrinks, to half at most (%lld)", (long long)sp.part_frags);
    sp = fresh_spec();
    verdict(sp, s, 100, Forms(), 4000);
    CHECK(sp.part_frags == 40, "events: to four fifths of what fits (%lld)", (long long)sp.part_frags);
    sp = fresh_spec();
    CHECK(verdict(sp, s, 100, Forms(), 8000).kind == Verdict::VOIDED, "events: items_max itself is enough");
    sp = fresh_spec();
    CHECK(verdict(sp, s, 1, Forms(), 100).kind == Verdict::FAILED, "events: one fragment cannot shrink");
  }
  {  // seeds: 2^31 hits shrink the part before anything else
    Spec sp = fresh_spec(); PassStatus s = quiet_status(); s.totals[TOT_SEEDS] = (1ULL << 31) - 1;
    CHECK(verdict(sp, s).kind == Verdict::ACCEPTED, "seeds: 2^31 - 1 hits are addressable");
    s.totals[TOT_SEEDS] = 1ULL << 31; s.stats[STAT_SMAX] = 1000;
    const Verdict v = verdict(sp = fresh_spec(), s, 1000);
    CHECK(v.kind == Verdict::SHRUNK && sp.part_frags == 500 && sp.smax == 256, "seeds: 2^31 hits shrink the part (%lld), nothing else", (long long)sp.part_frags);
    s.totals[TOT_SEEDS] = 1ULL << 33;
    verdict(sp = fresh_spec(), s, 1000);
    CHECK(sp.part_frags == 200, "seeds: to four fifths of what fits (%lld)", (long long)sp.part_frags);
    CHECK(verdict(sp = fresh_spec(), s, 1).kind == Verdict::FAILED, "seeds: one fragment cannot shrink");
  }
}

static void test_policy_wide_prefilter_scan() {
  // wide state: a part that needed it without the wide pass is void, and redo stays set
  Spec ms = fresh_spec(), sp = ms;
  PassStatus s = quiet_status(); s.counters[CNT_WIDE] = 3;
  Verdict v = verdict(sp, s);
  CHECK(v.kind == Verdict::VOIDED && v.miss && sp.redo, "wide state: void, redo set");
  spec_merge(ms, sp);
  sp = ms;
  CHECK(verdict(sp, s).kind == Verdict::ACCEPTED, "wide state: accepted once the wide pass ran");
  sp.redo = false; spec_merge(ms, sp);
  CHECK(ms.redo, "redo is sticky");
  // pre-filter: above 0.5 % merged fragments, sticky; l1_no_small only with the pre-filter AND the 256-thread class next to another
  const struct { uint32_t merged; Forms ran; bool pf, no_small; } cases[] = {
    {5, ran_with(true, 2, 256), false, false}, {6, ran_with(false, 2, 256), true, false}, {6, ran_with(true, 1, 256), true, false},
    {6, ran_with(true, 2, 512), true, false}, {6, ran_with(true, 2, 256), true, true}, {6, ran_with(true, 3, 256), true, true}};
  for (auto &c : cases) {
    sp = fresh_spec(); s = quiet_status(); s.counters[CNT_MERGED] = c.merged;
    verdict(sp, s, 1000, c.ran);
    CHECK(sp.l1_prefilter == c.pf && sp.l1_no_small == c.no_small, "pre-filter with %u merged, pf %d, %d classes from %d threads: %d %d", c.merged,
          (int)c.ran.prefilter, c.ran.n_l1, c.ran.l1_threads[0], (int)sp.l1_prefilter, (int)sp.l1_no_small);
  }
  ms = fresh_spec(); sp = ms; sp.l1_prefilter = sp.l1_no_small = true; spec_merge(ms, sp);
  sp = fresh_spec(); spec_merge(ms, sp);
  CHECK(ms.l1_prefilter && ms.l1_no_small, "l1_prefilter and l1_no_small are sticky");
  // the record's merge: bounds grow, part_frags shrinks, seed slots follow the latest pass
  ms = fresh_spec(); sp = ms; sp.smax = 100; sp.l_cap = 10; sp.part_frags = 1 << 20; sp.seed_slots = 1024; spec_merge(ms, sp);
  CHECK(ms.smax == 256 && ms.l_cap == 1 << 18 && ms.part_frags == 48 * 1024 && ms.seed_slots == 1024, "spec_merge");
  // accepted part: the shares and the loci of the part
  sp = fresh_spec(); s = quiet_status(); s.stats[STAT_SMALL] = 500; s.stats[STAT_MID] = 250; s.stats[STAT_TINY] = 100; s.loci_region[0] = 2000;
  v = verdict(sp, s);
  CHECK(sp.l1_small_share == 0.5f && sp.l1_mid_share == 0.25f && sp.l1_tiny_share == 0.1f && sp.l2_loci_last == 1024 && v.loci == 1024, "shares and loci");
  // sorted scan: from 1 024 x 64 loci of the last part
  sp = fresh_spec(); sp.l2_loci_last = 1024 * 64 - 1;
  CHECK(!scan_sorted(sp, -1) && scan_sorted(sp, 1), "sorted scan below 65 536 loci");
  sp.l2_loci_last = 1024 * 64;
  CHECK(scan_sorted(sp, -1) && !scan_sorted(sp, 0), "sorted scan from 65 536 loci");
  CHECK(!wide_events(510) && wide_events(511), "wide events from a bound of 511");
  CHECK(!l1_near(299999999, -1) && l1_near(300000000, -1) && l1_near(0, 1) && !l1_near(1LL << 40, 0), "FA_L1_NEAR");
  CHECK(frag_order_gate(true, false, 2, 64) && !frag_order_gate(true, false, 2, 63) && !frag_order_gate(true, false, 1, 1000) &&
        frag_order_gate(true, true, 1, 64) && !frag_order_gate(false, true, 5, 1000), "the gate of the workgroup order");
  // every SPEC_* flag voids
  for (uint32_t f = 1; f <= SPEC_LAST; f <<= 1) {
    sp = fresh_spec(); s = quiet_status(); s.pinfo[PI_FLAGS] = f;
    CHECK(verdict(sp, s).kind == Verdict::VOIDED, "flag %u voids the part", f);
  }
}

static void test_policy_l1_plan() {
  const uint32_t INF = 0xFFFFFFFFu;
  auto plan = [](uint32_t seed_slots, int64_t records = 0, const L1Knobs &k = L1Knobs(), float small = -1.0f, float mid = -1.0f, float tiny = -1.0f,
                 bool pf = false, bool no_small = false) {
    Spec sp = fresh_spec(); sp.seed_slots = seed_slots; sp.l1_small_share = small; sp.l1_mid_share = mid; sp.l1_tiny_share = tiny;
    sp.l1_prefilter = pf; sp.l1_no_small = no_small;
    return plan_l1(sp, records, k);
  };
  auto covers = [&](const L1Plan &p) {                          // the kept ranges cover [0, inf) without gaps
    bool ok = p.n >= 1 && p.c[0].n_lo == 0 && p.c[p.n - 1].n_hi == INF;
    for (int i = 0; i + 1 < p.n; i++) ok = ok && p.c[i].n_hi != INF && p.c[i + 1].n_lo == p.c[i].n_hi + 1;
    return ok;
  };
  auto shape = [](const L1Plan &p) { int v = 0; for (int i = 0; i < p.n; i++) v = v * 10 + (p.c[i].nt == 256 ? 1 : p.c[i].slots <= L1_MID_HITS ? 2 : 3); return v; };
  // the classes at the boundaries of L1_SMALL_HITS, L1_MID_HITS and the LDS cap (no shares seen: every class kept)
  CHECK(shape(plan(L1_SMALL_HITS)) == 1 && plan(L1_SMALL_HITS).c[0].slots == L1_SMALL_HITS, "one class up to L1_SMALL_HITS");
  CHECK(floor_log2(1) == 0 && floor_log2(1023) == 9 && floor_log2(1024) == 10 && floor_log2(2147483584) == 30, "floor_log2");
  CHECK(shape(plan(L1_SMALL_HITS + 1)) == 12 && plan(L1_SMALL_HITS + 1).c[1].n_lo == L1_SMALL_HITS + 1, "two classes above it");
  CHECK(shape(plan(L1_MID_HITS)) == 12 && shape(plan(L1_MID_HITS + 1)) == 123, "three classes above L1_MID_HITS");
  CHECK(plan(L1_MID_HITS + 1).c[2].slots == L1_MID_HITS + 1 && plan(L1_MID_HITS + 1).c[2].n_lo == L1_MID_HITS + 1, "the last class takes the need");
  CHECK(plan(1u << 20).need == lds_seed_cap_max(256) && plan(1u << 20).c[2].slots == L1_INPLACE_MAX * 512, "the LDS cap bounds the need");
  CHECK(plan(1000).seed_slots() == 1000 && plan(12000).seed_slots() == 12000 && plan(1u << 20).seed_slots() == L1_INPLACE_MAX * 512, "seed slots of the last class");
  // the pre-filter: from 3 x 10^8 records, or sticky, or forced
  CHECK(!plan(4096, 299999999).prefilter && plan(4096, 300000000).prefilter && plan(4096, 0, L1Knobs(), -1, -1, -1, true).prefilter, "pre-filter on");
  CHECK(!plan(4096, 1LL << 40, L1Knobs{0, -1.0f, 0.05f}).prefilter && plan(4096, 0, L1Knobs{1, -1.0f, 0.05f}).prefilter, "FA_L1_PREFILTER");
  // keep / fold: the small class with the pre-filter from 35 % small fragments, without from 50 % tiny ones; the middle class
  // from 5 % (or to carry the small ones, or when it is the last)
  const uint32_t two = 6000, three = 20000;
  CHECK(shape(plan(two, 0, L1Knobs(), 0.0f, 0.0f, 0.5f)) == 12 && shape(plan(two, 0, L1Knobs(), 1.0f, 0.0f, 0.49f)) == 2, "tiny share without the pre-filter");
  CHECK(shape(plan(two, 0, L1Knobs(), 0.35f, 0.0f, 0.0f, true)) == 12 && shape(plan(two, 0, L1Knobs(), 0.34f, 1.0f, 1.0f, true)) == 2, "small share with it");
  CHECK(shape(plan(three, 0, L1Knobs(), 0.0f, 0.05f, 1.0f)) == 123 && shape(plan(three, 0, L1Knobs(), 0.0f, 0.049f, 1.0f)) == 13, "middle share");
  CHECK(shape(plan(three, 0, L1Knobs(), 0.0f, 0.0f, 0.0f)) == 23, "the middle class carries the small ones");
  CHECK(shape(plan(three, 0, L1Knobs(), 1.0f, 1.0f, 1.0f, true, true)) == 23 && shape(plan(two, 0, L1Knobs(), 1.0f, 1.0f, 1.0f, false, true)) == 2, "l1_no_small folds the small class");
  CHECK(shape(plan(three, 0, L1Knobs{-1, 0.2f, 0.05f}, 0.2f, 1.0f, 0.0f, true, true)) == 123 &&
        shape(plan(three, 0, L1Knobs{-1, 0.2f, 0.05f}, 0.19f, 1.0f, 1.0f)) == 23, "FA_L1_THIN_SMALL overrides the rules");
  CHECK(shape(plan(three, 0, L1Knobs{-1, -1.0f, 0.5f}, -1.0f, 0.49f, -1.0f)) == 13 && shape(plan(three, 0, L1Knobs{-1, -1.0f, 0.0f}, -1.0f, 0.0f, -1.0f)) == 123,
        "FA_L1_THIN_MID");
  // every combination of shares, switches and overrides keeps [0, inf) covered
  int plans = 0;
  for (uint32_t need : {100u, L1_SMALL_HITS, L1_SMALL_HITS + 1, L1_MID_HITS, L1_MID_HITS + 1, 1u << 20})
    for (float sh : {-1.0f, 0.0f, 0.34f, 0.35f, 1.0f}) for (float md : {-1.0f, 0.0f, 0.05f, 1.0f}) for (float ty : {-1.0f, 0.0f, 0.5f})
      for (int pf = 0; pf < 2; pf++) for (int ns = 0; ns < 2; ns++)
        for (const L1Knobs &k : {L1Knobs(), L1Knobs{0, -1.0f, 0.05f}, L1Knobs{1, -1.0f, 0.05f}, L1Knobs{-1, 0.3f, 0.05f}, L1Knobs{-1, -1.0f, 0.9f}}) {
          const L1Plan p = plan(need, 0, k, sh, md, ty, pf, ns);
          plans++;
          CHECK(covers(p), "plan for %u slots (shares %.2f %.2f %.2f, pf %d, no_small %d) leaves a gap", need, sh, md, ty, pf, ns);
        }
  CHECK(plans == 6 * 5 * 4 * 3 * 2 * 2 * 5, "plans checked");
}

static void test_policy_fuse_backoff() {
  Spec ms = fresh_spec();
  const int skips[] = {0, 1, 3, 7, 15, 31, 63, 63, 63};
  for (int want : skips) { fuse_overflowed(ms); CHECK(ms.fuse_skip == want, "skip after consecutive overflows: %d (want %d)", ms.fuse_skip, want); }
  fuse_accepted(ms, false, true);
  CHECK(ms.fuse_skip == 62 && ms.fuse_penalty == 64, "an accepted unfused part serves a pass of the back-off");
  fuse_accepted(ms, false, false);
  CHECK(ms.fuse_skip == 62, "the forced repeat of an overflow serves nothing");
  fuse_accepted(ms, true, false);
  CHECK(ms.fuse_penalty == 0, "an accepted fused part clears the penalty");
  fuse_overflowed(ms);
  CHECK(ms.fuse_penalty == 1 && ms.fuse_skip == 0, "and the next overflow starts over");
  ms.fuse_skip = 2;
  for (int want : {1, 0, 0}) { fuse_accepted(ms, false, true); CHECK(ms.fuse_skip == want, "countdown %d (want %d)", ms.fuse_skip, want); }
}

static void test_policy_frag_order() {
  auto is_perm = [](const std::vector<int32_t> &o, int64_t F) {
    std::vector<int> seen((size_t)F, 0);
    int64_t real = 0;
    for (int32_t x : o) { if (x == -1) continue; if (x < 0 || x >= F || seen[(size_t)x]++) return false; real++; }
    return real == F && o.size() % 8 == 0;
  };
  std::vector<int32_t> out;
  // one genome: eight contiguous runs, from 64 fragments on
  std::vector<int64_t> lo = {0, 63};
  CHECK(build_frag_order(lo.data(), 0, 0, 63, out) == 0, "one genome under 64 fragments: identity order");
  lo = {0, 100};
  CHECK(build_frag_order(lo.data(), 0, 0, 100, out) == 104 && is_perm(out, 100) && out[0] == 0 && out[1] == 13 && out[8] == 1, "one genome: runs of 13");
  // several genomes: fewer than 8 offset groups
  lo = {0, 7, 14, 21, 28};
  CHECK(build_frag_order(lo.data(), 0, 0, 28, out) == 0, "7 offsets: identity order");
  lo = {0, 8, 16, 24, 32, 40, 48, 56, 64};
  CHECK(build_frag_order(lo.data(), 0, 0, 64, out) == 64 && is_perm(out, 64), "8 offsets of 8 genomes: no padding");
  // padding above 15 %: 9 groups of 10 on 8 XCDs (one XCD takes two groups)
  lo.clear(); for (int i = 0; i <= 10; i++) lo.push_back(9 * i);
  CHECK(build_frag_order(lo.data(), 0, 0, 90, out) == 0, "9 groups of 10: too much padding");
  // 8 groups of 10 and a ninth of 2 (two genomes one fragment longer): 12 x 8 slots for 82 fragments is 17 % padding; with a
  // ninth group of 1, 11 x 8 for 81 is 8.6 %
  lo = {0, 9, 18, 26, 34, 42, 50, 58, 66, 74, 82};
  CHECK(build_frag_order(lo.data(), 0, 0, 82, out) == 0, "17 %% padding: identity order");
  lo = {0, 9, 17, 25, 33, 41, 49, 57, 65, 73, 81};
  CHECK(build_frag_order(lo.data(), 0, 0, 81, out) == 88 && is_perm(out, 81), "8.6 %% padding: the XCD order");
  // 16 groups of 10 genomes, from the third genome of the batch and part-way into it
  lo.clear(); for (int i = 0; i <= 12; i++) lo.push_back(16 * i);
  CHECK(build_frag_order(lo.data(), 2, 32, 192, out) == 160 && is_perm(out, 160), "16 offsets of 10 genomes");
  // offsets dealt to XCDs: within 15 % padding, always a permutation
  lo = {0, 20, 39, 60, 80, 99, 120};
  const uint32_t n = build_frag_order(lo.data(), 0, 0, 120, out);
  CHECK(n == 0 || (is_perm(out, 120) && n * 1.0 <= 1.15 * 120 + 7), "uneven genomes: %u", n);
}

// ---- the contig bookkeeping of ingest (fa_ingest.h) against restatements that follow _fastani.pyx one contig at a time ----
typedef std::vector<std::vector<int64_t>> GenomeLens;             // contig lengths, genome by genome
static fa_params ingest_params(int k, int w, int frag, bool protein = false) {
  fa_params P; memset(&P, 0, sizeof P);
  P.kmer_size = k; P.window_size = w; P.fragment_length = frag; P.alphabet_size = protein ? 20 : 4;
  return P;
}
static const int64_t kLenMax = (1LL << 31) - 1;
// the lengths at which a rule turns: zero, the admission rule, whole fragments, the limit
static std::vector<int64_t> edge_lengths(const fa_params &P) {
  const int64_t lo = std::min(P.window_size, P.kmer_size), hi = std::max(P.window_size, P.kmer_size), f = P.fragment_length;
  return {0, lo - 1, lo, hi - 1, hi, f - 1, f, f + 1, 2 * f - 1, kLenMax};
}
// a leading and a trailing empty genome, every edge length, a genome of short contigs only, empty genomes in between, random ones
static GenomeLens ingest_genomes(const fa_params &P, uint64_t seed) {
  std::mt19937_64 rng(seed);
  const std::vector<int64_t> edges = edge_lengths(P);
  GenomeLens g;
  g.push_back({});
  g.push_back(edges);
  g.push_back({0, std::min(P.window_size, P.kmer_size) - 1, 0});
  for (int i = 0; i < 12; i++) {
    std::vector<int64_t> contigs;
    const int n = i % 4 == 3 ? 0 : 1 + (int)(rng() % 7);
    for (int c = 0; c < n; c++) contigs.push_back(rng() % 3 == 0 ? (int64_t)(rng() % (5 * (uint64_t)P.fragment_length)) : edges[rng() % (edges.size() - 1)]);
    g.push_back(contigs);
  }
  g.push_back({});
  return g;
}
static void flatten(const GenomeLens &g, size_t first, size_t count, std::vector<int64_t> &lens, std::vector<int32_t> &genome) {
  lens.clear(); genome.clear();
  for (size_t i = 0; i < count; i++) for (int64_t l : g[first + i]) { lens.push_back(l); genome.push_back((int32_t)i); }
}

// Sketch._add_draft, one genome (_fastani.pyx:610-690); `carried`: what earlier contigs without a genome have left
struct PlainBook { int64_t counter = 0; uint64_t carried = 0; std::vector<uint64_t> lengths; std::vector<int32_t> by_file, sketched; std::vector<int64_t> shorts; };
static void plain_add_draft(PlainBook &b, const fa_params &P, const std::vector<int64_t> &contigs) {
  uint64_t total = b.carried;
  int64_t shorts = 0;
  for (int64_t len : contigs) {
    if (len < P.window_size || len < P.kmer_size) shorts++;       // :648, :670-677
    else b.sketched.push_back((int32_t)b.counter);
    total += (uint64_t)(len - len % P.fragment_length);           // :680
    b.counter++;                                                  // :683
  }
  b.carried = 0;
  b.lengths.push_back(total);                                     // :687
  b.by_file.push_back((int32_t)b.counter);                        // :690
  b.shorts.push_back(shorts);
}
static bool same_book(const RefBook &a, const RefBook &b) {
  return a.counter == b.counter && a.cur_total == b.cur_total && a.lengths == b.lengths && a.seqs_by_file == b.seqs_by_file && a.pending_contig == b.pending_contig;
}
static bool book_is(const RefBook &a, const PlainBook &w) {
  return a.counter == w.counter && a.cur_total == w.carried && a.lengths == w.lengths && a.seqs_by_file == w.by_file && a.pending_contig == w.sketched;
}
// does `fn` fail with `code` and exactly `text`?
template <class Fn> static bool refused(Fn fn, int code, const char *text) {
  try { fn(); } catch (const Error &e) { return e.code == code && std::string(e.what()) == text; }
  return false;
}

static void test_ingest_reference_roads(const fa_params &P, uint64_t seed) {
  const GenomeLens genomes = ingest_genomes(P, seed);
  PlainBook want;
  for (auto &g : genomes) plain_add_draft(want, P, g);
  std::vector<int64_t> lens; std::vector<int32_t> genome;
  // contig by contig with end_genome (add_draft)
  RefBook one;
  for (auto &g : genomes) {
    for (int64_t len : g) { RefStage add(one, OpenGenome::FOLD); const bool in = add.contig(P, len); add.commit(one); CHECK(in == ref_admitted(P, len), "contig(%lld) and the admission rule", (long long)len); }
    RefStage add(one, OpenGenome::FOLD); add.end_genome(); add.commit(one);
  }
  CHECK(book_is(one, want), "contig by contig: the book differs from the restatement (k %d w %d)", P.kmer_size, P.window_size);
  // all at once (add_genomes)
  RefBook all;
  {
    flatten(genomes, 0, genomes.size(), lens, genome);
    std::vector<int64_t> admitted_at;
    RefStage add(all, OpenGenome::REFUSE, (int64_t)genomes.size());
    add.genomes(P, lens.data(), genome.data(), (int64_t)lens.size(), (int32_t)genomes.size(), [&](int64_t c) { admitted_at.push_back(c); });
    bool packed = false;
    add.commit(all, [&] { packed = true; CHECK(all.counter == 0 && all.lengths.empty(), "the packer runs before anything is inserted"); });
    CHECK(packed && add.n_short == want.shorts, "all at once: packer call and short counts");
    CHECK(admitted_at.size() == want.sketched.size(), "all at once: %zu admitted vs %zu", admitted_at.size(), want.sketched.size());
    for (size_t i = 0; i < admitted_at.size() && i < want.sketched.size(); i++) CHECK(admitted_at[i] == want.sketched[i], "all at once: admitted contig %zu", i);
  }
  CHECK(book_is(all, want), "all at once: the book differs from the restatement");
  // file by file (add_fasta): one genome per call, no genome numbers
  RefBook files;
  for (size_t i = 0; i < genomes.size(); i++) {
    RefStage add(files, OpenGenome::FOLD);
    add.genomes(P, genomes[i].data(), nullptr, (int64_t)genomes[i].size(), 1, [](int64_t) {});
    add.commit(files);
    CHECK(add.n_short.size() == 1 && add.n_short[0] == want.shorts[i], "file by file: short count of genome %zu", i);
  }
  CHECK(book_is(files, want), "file by file: the book differs from the restatement");
  // packed files, a few per call (add_fasta_many / add_packed)
  RefBook packed;
  for (size_t i = 0; i < genomes.size(); i += 4) {
    const size_t n = std::min<size_t>(4, genomes.size() - i);
    flatten(genomes, i, n, lens, genome);
    RefStage add(packed, OpenGenome::REFUSE, (int64_t)n);
    add.genomes(P, lens.data(), genome.data(), (int64_t)lens.size(), (int32_t)n, [](int64_t) {});
    add.commit(packed);
  }
  CHECK(book_is(packed, want), "packed files: the book differs from the restatement");
  CHECK(same_book(one, all) && same_book(all, files) && same_book(files, packed), "the four roads leave equal books");
}

static void test_ingest_reference_refusals(const fa_params &P) {
  const char *too_long = "contig length must be below 2^31", *bad_genome = "contig_genome must be non-decreasing and < n_genomes",
             *open = "a genome is still open (add_contig without end_genome)";
  const int64_t f = P.fragment_length;
  RefBook book;
  { RefStage add(book, OpenGenome::FOLD); const int64_t l[3] = {3 * f, 0, f + 1}; add.genomes(P, l, nullptr, 3, 1, [](int64_t) {}); add.commit(book); }
  const RefBook before = book;
  auto road = [&](std::vector<int64_t> lens, std::vector<int32_t> genome, int32_t n_genomes) {
    RefStage add(book, OpenGenome::REFUSE, n_genomes);
    add.genomes(P, lens.data(), genome.data(), (int64_t)lens.size(), n_genomes, [](int64_t) {});
    add.commit(book);
  };
  CHECK(refused([&] { road({f, 2 * f, 1LL << 31}, {0, 0, 1}, 2); }, FA_ERR_INVALID, too_long) && same_book(book, before), "2^31 is refused, the book untouched");
  CHECK(refused([&] { road({f, 2 * f, -1}, {0, 0, 1}, 2); }, FA_ERR_INVALID, too_long) && same_book(book, before), "-1 is refused, the book untouched");
  CHECK(refused([&] { RefStage add(book, OpenGenome::FOLD); add.contig(P, 1LL << 31); add.commit(book); }, FA_ERR_INVALID, too_long) && same_book(book, before), "one contig of 2^31");
  CHECK(refused([&] { road({f, 2 * f, f, f}, {0, 1, 1, 0}, 2); }, FA_ERR_INVALID, bad_genome) && same_book(book, before), "a decreasing contig_genome");
  CHECK(refused([&] { road({f, 2 * f, f, f}, {0, 1, 1, 2}, 2); }, FA_ERR_INVALID, bad_genome) && same_book(book, before), "contig_genome >= n_genomes");
  CHECK(refused([&] { road({f}, {-1}, 2); }, FA_ERR_INVALID, bad_genome) && same_book(book, before), "a negative contig_genome");
  // a packer that fails: the book is as before
  bool threw = false;
  try {
    RefStage add(book, OpenGenome::FOLD); const int64_t l[2] = {f, 5 * f};
    add.genomes(P, l, nullptr, 2, 1, [](int64_t) {});
    add.commit(book, [] { throw std::bad_alloc(); });
  } catch (const std::bad_alloc &) { threw = true; }
  CHECK(threw && same_book(book, before), "a failing packer leaves the book as it was");
  // a genome that add_contig left open: folded by add_fasta's policy, refused by the other
  { RefStage add(book, OpenGenome::FOLD); add.contig(P, 2 * f + 1); add.commit(book); }
  CHECK(book.cur_total == (uint64_t)(2 * f) && book.counter == before.counter + 1 && book.lengths == before.lengths, "an open genome carries its length");
  const RefBook opened = book;
  CHECK(refused([&] { road({f}, {0}, 1); }, FA_ERR_INVALID, open) && same_book(book, opened), "an open genome is refused by the batch roads");
  CHECK(refused([&] { road({}, {}, 1); }, FA_ERR_INVALID, open) && same_book(book, opened), "... also by a batch of one genome without contigs");
  road({}, {}, 0);
  CHECK(same_book(book, opened), "a batch road that brings no genome changes nothing beside an open genome");
  { RefStage add(book, OpenGenome::FOLD); const int64_t l[2] = {f, 3 * f - 1}; add.genomes(P, l, nullptr, 2, 1, [](int64_t) {}); add.commit(book); }
  CHECK(book.cur_total == 0 && book.lengths.back() == (uint64_t)(5 * f) && book.seqs_by_file.back() == (int32_t)before.counter + 3, "add_fasta folds the open genome in");
}

// Mapper._query_draft over a batch (_fastani.pyx:985, 1061-1105), every fragment written out
struct PlainBatch { std::vector<int32_t> frag_query, frag_qseq; std::vector<int64_t> genome_frag_lo, contig_frag_lo; std::vector<uint64_t> tf, tl; std::vector<int32_t> ns; uint64_t bases_in_frags = 0; size_t store = 0; };
static PlainBatch plain_batch(const fa_params &P, const GenomeLens &genomes) {
  PlainBatch b;
  const int64_t frag = P.fragment_length;
  for (size_t g = 0; g < genomes.size(); g++) {
    b.genome_frag_lo.push_back((int64_t)b.frag_query.size());
    uint64_t nfrag = 0, length = 0; int32_t shorts = 0;
    for (int64_t len : genomes[g]) {
      if (len < P.window_size && len < P.kmer_size && len < frag) { shorts++; continue; }              // :1061-1070
      if (len >= frag) b.contig_frag_lo.push_back((int64_t)b.frag_query.size());
      for (int64_t i = 0; (i + 1) * frag <= len; i++) { b.frag_query.push_back((int32_t)g); b.frag_qseq.push_back((int32_t)(nfrag + (uint64_t)i)); }   // :985
      const int64_t n = len / frag;                                                                  // :1097
      nfrag += (uint64_t)n; length += (uint64_t)len;                                                  // :1104, :1105
      b.bases_in_frags += (uint64_t)(n * frag);
      if (n > 0) b.store += (size_t)((n * frag + 63) / 64 * 64);
    }
    b.tf.push_back(nfrag); b.tl.push_back(length); b.ns.push_back(shorts);
  }
  b.genome_frag_lo.push_back((int64_t)b.frag_query.size());
  return b;
}
static const int kTilePositions = 1024;                            // TILE and sizeof(Tile) of fa_sketch.hip.h
static const size_t kTileBytes = 32;
static void check_layout(const BatchPlan &b, bool protein, int32_t n_genomes, const char *what) {
  const BatchLayout::Part *parts[7] = {&b.at.packed, &b.at.bytes, &b.at.tiles, &b.at.frag_tile_lo, &b.at.frag_query, &b.at.frag_qseq, &b.at.total_frag};
  const size_t need[7] = {protein ? 0 : b.bases / 4 + 4, protein ? b.bases + 1 : 0, (size_t)b.ntiles * kTileBytes, ((size_t)b.F + 1) * 4, (size_t)b.F * 4, (size_t)b.F * 4, (size_t)n_genomes * 4};
  size_t end = 0;
  for (int i = 0; i < 7; i++) {
    CHECK(parts[i]->at % 16 == 0 && parts[i]->at == end, "%s: part %d starts at %zu, the one before ends at %zu", what, i, parts[i]->at, end);
    CHECK(parts[i]->bytes >= need[i], "%s: part %d holds %zu bytes, %zu are written", what, i, parts[i]->bytes, need[i]);
    end = parts[i]->at + parts[i]->bytes;
  }
  CHECK(end == b.at.image_bytes, "%s: the parts end at %zu, the image at %zu", what, end, b.at.image_bytes);
  CHECK((protein ? b.at.packed.bytes : b.at.bytes.bytes) == 0, "%s: the image of the other alphabet is empty", what);
}
static void test_ingest_batch_plan(const fa_params &P, uint64_t seed) {
  GenomeLens genomes = ingest_genomes(P, seed);
  const int64_t min_len = std::min<int64_t>(std::min(P.window_size, P.kmer_size), P.fragment_length);
  if (min_len < P.fragment_length) genomes.push_back({min_len, P.fragment_length - 1});     // mapped, but no fragment
  const bool protein = P.alphabet_size != 4;
  const PlainBatch want = plain_batch(P, genomes);
  std::vector<int64_t> lens; std::vector<int32_t> genome;
  flatten(genomes, 0, genomes.size(), lens, genome);
  const BatchPlan b = plan_batch(P, lens.data(), genome.data(), (int64_t)lens.size(), (int32_t)genomes.size(), kTilePositions, kTileBytes);
  CHECK(b.genome_frag_lo == want.genome_frag_lo && b.contig_frag_lo == want.contig_frag_lo, "batch plan: fragment ranges of genomes and contigs");
  CHECK(b.total_fragments == want.tf && b.total_length == want.tl && b.n_short == want.ns, "batch plan: per-genome counters");
  CHECK(b.F == (int64_t)want.frag_query.size() && b.total_bases == want.bases_in_frags && b.bases == want.store, "batch plan: F %lld, bases %llu", (long long)b.F, (unsigned long long)b.total_bases);
  const int64_t npos = (int64_t)P.fragment_length - P.kmer_size + 1, per = npos > 0 ? (npos + kTilePositions - 1) / kTilePositions : 0;
  CHECK(b.tiles_per_frag == per && b.ntiles == b.F * per, "batch plan: %lld tiles", (long long)b.ntiles);
  if (min_len < P.fragment_length) CHECK(b.n_short.back() == 0 && b.total_fragments.back() == 0 && b.total_length.back() == (uint64_t)(min_len + P.fragment_length - 1), "a contig below one fragment counts in the length only");
  // the per-fragment tables as fill_genomes writes them from the jobs
  std::vector<int32_t> frag_query((size_t)b.F, -1), frag_qseq((size_t)b.F, -1);
  CHECK(b.jobs.size() == b.use_len.size() && b.jobs.size() == b.contig_frag_lo.size(), "batch plan: one entry per contig that holds fragments");
  for (size_t j = 0; j < b.jobs.size(); j++) {
    const ContigJob &cj = b.jobs[j];
    CHECK(cj.si == (int64_t)j && cj.gi == genome[(size_t)cj.c] && b.use_len[j] == cj.nfrag * P.fragment_length && b.use_len[j] <= lens[(size_t)cj.c] && cj.nf0 + cj.nfrag <= b.F, "batch plan: job %zu", j);
    if (cj.nf0 + cj.nfrag > b.F) break;
    for (int64_t i = 0; i < cj.nfrag; i++) { frag_query[(size_t)(cj.nf0 + i)] = cj.gi; frag_qseq[(size_t)(cj.nf0 + i)] = (int32_t)(cj.q0 + i); }
  }
  CHECK(frag_query == want.frag_query && frag_qseq == want.frag_qseq, "batch plan: frag_query / frag_qseq");
  check_layout(b, protein, (int32_t)genomes.size(), protein ? "protein batch" : "batch");
}
static void test_ingest_batch_limits() {
  fa_params P = ingest_params(16, 24, 3000);
  const char *bad_genome = "contig_genome must be non-decreasing and < n_genomes", *too_many = "too many fragments in one batch";
  BatchPlan b = plan_batch(P, nullptr, nullptr, 0, 3, kTilePositions, kTileBytes);
  CHECK(b.F == 0 && b.ntiles == 0 && b.jobs.empty() && b.genome_frag_lo == std::vector<int64_t>(4, 0) && b.n_short == std::vector<int32_t>(3, 0), "three genomes without contigs");
  check_layout(b, false, 3, "batch without contigs");
  b = plan_batch(P, nullptr, nullptr, 0, 0, kTilePositions, kTileBytes);
  CHECK(b.F == 0 && b.genome_frag_lo == std::vector<int64_t>(1, 0) && b.total_fragments.empty(), "no genomes");
  check_layout(b, false, 0, "batch without genomes");
  const int64_t some[3] = {3000, 9000, 3000};
  const int32_t down[3] = {0, 1, 0}, over[3] = {0, 1, 2};
  CHECK(refused([&] { plan_batch(P, some, down, 3, 2, kTilePositions, kTileBytes); }, FA_ERR_INVALID, bad_genome), "a decreasing contig_genome in a batch");
  CHECK(refused([&] { plan_batch(P, some, over, 3, 2, kTilePositions, kTileBytes); }, FA_ERR_INVALID, bad_genome), "contig_genome >= n_genomes in a batch");
  CHECK(refused([&] { plan_batch(P, some, nullptr, 1, 0, kTilePositions, kTileBytes); }, FA_ERR_INVALID, bad_genome), "a contig without a genome");
  // F: 2^31 - 2 fragments fit, 2^31 - 1 do not (one tile per fragment)
  P = ingest_params(1, 1, 1);
  int64_t len = kLenMax - 1;
  b = plan_batch(P, &len, nullptr, 1, 1, kTilePositions, kTileBytes);
  CHECK(b.F == kLenMax - 1 && b.ntiles == b.F && b.jobs.size() == 1, "2^31 - 2 fragments");
  check_layout(b, false, 1, "largest batch");
  len = kLenMax;
  CHECK(refused([&] { plan_batch(P, &len, nullptr, 1, 1, kTilePositions, kTileBytes); }, FA_ERR_UNSUPPORTED, too_many), "2^31 - 1 fragments are refused");
  const int64_t two[2] = {kLenMax - 1, 1};
  CHECK(refused([&] { plan_batch(P, two, nullptr, 2, 1, kTilePositions, kTileBytes); }, FA_ERR_UNSUPPORTED, too_many), "... from two contigs as well");
  // tiles: two per fragment; 2^30 - 1 fragments fit, 2^30 do not
  P = ingest_params(16, 24, 2063);
  const int64_t per_contig = kLenMax / 2063;
  for (int64_t F : {(1LL << 30) - 1, 1LL << 30}) {
    std::vector<int64_t> lens;
    for (int64_t left = F; left > 0; left -= std::min(left, per_contig)) lens.push_back(std::min(left, per_contig) * 2063 + 7);
    if (F < (1LL << 30)) {
      b = plan_batch(P, lens.data(), nullptr, (int64_t)lens.size(), 1, kTilePositions, kTileBytes);
      CHECK(b.F == F && b.tiles_per_frag == 2 && b.ntiles == (1LL << 31) - 2, "2^31 - 2 tiles");
    } else CHECK(refused([&] { plan_batch(P, lens.data(), nullptr, (int64_t)lens.size(), 1, kTilePositions, kTileBytes); }, FA_ERR_UNSUPPORTED, too_many), "2^31 tiles are refused");
  }
}
static void test_ingest() {
  // w > k (the default sketch) and w < k; the second also at 200-base fragments, where a mapped contig may hold no fragment
  const fa_params settings[] = {ingest_params(16, 24, 3000), ingest_params(21, 15, 200), ingest_params(5, 1, 100, true)};
  uint64_t seed = 4100;
  for (const fa_params &P : settings) {
    test_ingest_reference_roads(P, seed++);
    test_ingest_reference_refusals(P);
    test_ingest_batch_plan(P, seed++);
  }
  test_ingest_batch_limits();
}

int main() {
  for (int width : {1, 2, 4}) test_packer(false, width, 1);
  test_packer(true, 1, 1);
  test_packer(false, 1, 4);                                      // four concurrent clients on the one thread pool
  test_packer(true, 4, 4);
  test_fasta(1);
  test_fasta(4);
  test_fasta_packed(false);
  test_fasta_packed(true);
  test_stats();
  test_lease(8);
  test_spin();
  test_policy_sketch_bound();
  test_policy_seed_slots();
  test_policy_loci_events_seeds();
  test_policy_wide_prefilter_scan();
  test_policy_l1_plan();
  test_policy_fuse_backoff();
  test_policy_frag_order();
  test_ingest();
  // an item that throws inside the pool reaches the caller, and the pool keeps working afterwards
  bool caught = false;
  try { HostPool::get().parallel_for(64, [](size_t i) { if (i == 13) throw Error(FA_ERR_NOMEM, "item"); }); } catch (const Error &e) { caught = e.code == FA_ERR_NOMEM; }
  CHECK(caught, "an exception inside a pool item is re-raised on the caller");
  std::atomic<size_t> sum{0};
  HostPool::get().parallel_for(1000, [&](size_t i) { sum += i; });
  CHECK(sum == 499500, "pool after the exception");
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  printf("host pieces: all checks passed\n");
  return 0;
}
