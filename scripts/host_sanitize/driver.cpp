// Host-side pieces of libfastani_hip under AddressSanitizer + UBSan, and (separately) ThreadSanitizer, on the CPU:
//   the 2-bit packer (fa_host.h: AVX2 path, scalar exception path, wide characters, protein bytes) on the persistent thread
//   pool, the memory-mapped FASTA reader (fa_fasta.h), the statistics tables (fa_stats.h), the workspace lease and the
//   pinned-word spin (fa_lease.h), the policy of a query pass (fa_policy.h: every rule at the boundaries where it turns).  Inputs: the edge cases of tests/test_gpu_parity.py::test_minimizer_streams and
//   tests/test_fasta.py, plus four concurrent clients.  No HIP: these headers are what fa_engine.hip includes for the same jobs.
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
