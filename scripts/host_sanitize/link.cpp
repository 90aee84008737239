// The arithmetic of fa_table_linkage (pyfastani_amd/csrc/fa_link.h) at the ends of its range, on the CPU: build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all link.cpp  and run.
//
// Under UBSan a signed overflow in a sum, a product or the cut-off test is a finding of its own.  The largest case the
// library admits is 2^18 genomes: two clusters of 2^17, every pair present at identity 128 or every pair missing at the
// largest `missing`, against the largest cut-off the driver passes on (LINK_MAX_W + 1).  The order is also held against a
// second comparison that divides instead of multiplying (quotient, then remainders by cross products that fit 128 bits).
// The merge list of fa_table_dendrogram / fa_dendrogram_cut: what counts as a merge, its candidate and the cut-off of a float.
// The medoids of fa_table_medoids: the bonus, S, T, the key and the relation at the ends of their range.
#include <cstdint>
#include <cstdio>

#include "../../pyfastani_amd/csrc/fa_link.h"

static int failures = 0;
#define CHECK(cond, ...) \
  do { if (!(cond)) { if (failures++ < 20) { fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static uint64_t rng_state = 88172645463325252ULL;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// s1 / n1 against s2 / n2 without the 128-bit product of the sums: 1, 0 or 2 (equal averages)
static int by_division(const fa::LinkCand &a, const fa::LinkCand &b) {
  const long long qa = a.s / a.n, qb = b.s / b.n;
  if (qa != qb) return qa > qb ? 1 : 0;
  const unsigned __int128 x = (unsigned __int128)(a.s % a.n) * (unsigned long long)b.n, y = (unsigned __int128)(b.s % b.n) * (unsigned long long)a.n;
  return x == y ? 2 : x > y ? 1 : 0;
}

int main() {
  using namespace fa;
  CHECK(link_fixed(0.0) == 0 && link_fixed(128.0) == LINK_MAX_W && link_fixed(95.0) == 95LL << 20, "fixed point of round values");
  CHECK(link_fixed(0.5 / LINK_SCALE) == 0 && link_fixed(1.5 / LINK_SCALE) == 2 && link_fixed(2.5 / LINK_SCALE) == 2, "ties go to even");
  CHECK(link_identity_ok(0.0) && link_identity_ok(-0.0) && link_identity_ok(128.0), "the ends of the identity range");
  CHECK(!link_identity_ok(-1e-300) && !link_identity_ok(128.0000001) && !link_identity_ok(0.0 / 0.0), "outside it, and NaN");

  const long long half = (long long)LINK_MAX_GENOMES / 2, pairs = half * half;                  // 2^34
  const LinkSum full{LINK_MAX_W * pairs, pairs}, none{0, 0};
  const long long s_full = link_s(full, pairs, LINK_MAX_W), s_none = link_s(none, pairs, LINK_MAX_W);
  CHECK(s_full == LINK_MAX_W * pairs && s_none == s_full && s_full < (1LL << 62), "the largest sums stay below 2^62");
  CHECK(!link_passes(s_full, pairs, LINK_MAX_W + 1) && link_passes(s_full, pairs, LINK_MAX_W), "the largest cut-off");
  const LinkCand top{s_full, pairs, 0, 1}, below{s_full - 1, pairs, 0, 2}, tied{LINK_MAX_W * (pairs - 1), pairs - 1, 2, 3};
  CHECK(link_order(top, below) == 1 && link_order(below, top) == 0, "one unit of the sum decides");
  CHECK(link_order(top, tied) == 1 && link_order(tied, top) == 0 && link_order(top, top) == 2, "equal averages: the labels decide");
  const LinkCand nothing{0, 0, 0, 0};
  CHECK(link_better(top, nothing) && !link_better(nothing, top) && !link_better(nothing, nothing) && !link_better(top, top), "none comes last");

  // the merge list (fa_table_dendrogram, fa_dendrogram_cut): what is a merge, its candidate, and the cut-off of a float
  const int32_t n_max = LINK_MAX_GENOMES;
  CHECK(link_merge_ok(0, 1, 1, 1, 0, 1, 2) && link_merge_ok(0, n_max - 1, n_max / 2, n_max / 2, s_full, pairs, n_max), "the smallest and the largest merge");
  CHECK(!link_merge_ok(-1, 1, 1, 1, 0, 1, 2) && !link_merge_ok(1, 1, 1, 1, 0, 1, 2) && !link_merge_ok(2, 1, 1, 1, 0, 1, 3) && !link_merge_ok(0, 2, 1, 1, 0, 1, 2),
        "labels out of order or out of range");
  CHECK(!link_merge_ok(0, 1, 0, 1, 0, 1, 2) && !link_merge_ok(0, 1, 1, -1, 0, 1, 2) && !link_merge_ok(0, 1, 2, 1, 0, 1, 2), "sizes below 1 or beyond the genomes");
  CHECK(!link_merge_ok(0, 1, INT32_MAX, INT32_MAX, 0, 1, n_max) && !link_merge_ok(0, INT32_MAX, 1, 1, 0, 1, INT32_MAX), "the largest int32 in a size or a label");
  CHECK(!link_merge_ok(0, 1, 1, 1, -1, 1, 2) && !link_merge_ok(0, 1, 1, 1, 0, 0, 2) && !link_merge_ok(0, 1, 1, 1, INT64_MIN, INT64_MIN, 2), "a negative sum, no present pair");
  CHECK(link_merge_ok(0, 1, 1, 1, INT64_MAX, INT64_MAX, 2), "the largest sum is admitted: the cut compares it, it does not multiply it");
  const LinkCand widest = link_merge_cand(0, n_max - 1, n_max / 2, n_max / 2, s_full);
  CHECK(widest.n == pairs && widest.s == s_full && widest.lo == 0 && widest.hi == n_max - 1, "the candidate of the largest merge");
  CHECK(link_order(top, widest) == 1 && link_order(widest, top) == 0 && link_passes(widest.s, widest.n, link_cutoff(128.0f)) && !link_passes(widest.s, widest.n, link_cutoff(128.5f)),
        "the largest merge against the largest cut-offs");
  CHECK(link_passes(INT64_MAX, pairs, link_cutoff(3.0e38f)) && !link_passes(0, pairs, link_cutoff(1.0e-6f)) && link_passes(0, pairs, link_cutoff(0.0f)),
        "the cut-off test at the ends of s");
  CHECK(link_cutoff(0.0f) == 0 && link_cutoff(-0.0f) == 0 && link_cutoff(95.0f) == 95LL << 20 && link_cutoff(128.0f) == LINK_MAX_W, "cut-offs of round values");
  CHECK(link_cutoff(128.00001f) == LINK_MAX_W + 1 && link_cutoff(3.4e38f) == LINK_MAX_W + 1 && link_cutoff(INFINITY) == LINK_MAX_W + 1, "the clamp, infinity included");
  CHECK(link_cutoff(1.0f) == link_cutoff(1.00000012f), "two float32 with one fixed-point value");

  // centrality and medoids (fa_table_medoids): the bonus, S, T and the relation at the ends of their range -- a cluster of 2^18
  // genomes, every pair at 128 or every pair missing at 128, the largest bonus of either sign
  const long long m_max = LINK_MAX_GENOMES;
  CHECK(medoid_bonus_ok(32768.0) && medoid_bonus_ok(-32768.0) && medoid_bonus_ok(-0.0), "the ends of the bonus range");
  CHECK(!medoid_bonus_ok(32768.01) && !medoid_bonus_ok(-1e300) && !medoid_bonus_ok(0.0 / 0.0), "outside it, and NaN");
  CHECK(medoid_qb(32768.0) == 1LL << 35 && medoid_qb(-32768.0) == -(1LL << 35) && medoid_qb(0.5 / LINK_SCALE) == 0 && medoid_qb(1.5 / LINK_SCALE) == 2 &&
        medoid_qb(-1.5 / LINK_SCALE) == -2, "the fixed-point bonus, ties to even");
  const long long s_all = medoid_s(LINK_MAX_W * (m_max - 1), m_max - 1, m_max, LINK_MAX_W), s_missing = medoid_s(0, 0, m_max, LINK_MAX_W);
  CHECK(s_all == LINK_MAX_W * (m_max - 1) && s_missing == s_all && s_all < (1LL << 46) && medoid_s(0, 0, 1, LINK_MAX_W) == 0, "the largest S stays below 2^46");
  const long long t_top = medoid_t(s_all, medoid_qb(32768.0), m_max), t_bottom = medoid_t(0, medoid_qb(-32768.0), m_max);
  CHECK(t_top < (1LL << 54) && t_bottom > -(1LL << 54) && medoid_t(s_all, medoid_qb(32768.0), 1) == s_all, "|T| stays below 2^54");
  CHECK(medoid_key(t_bottom) < medoid_key(-1) && medoid_key(-1) < medoid_key(0) && medoid_key(0) < medoid_key(t_top) && medoid_key(t_bottom) != 0,
        "the key keeps the order across the sign and is never 0");
  CHECK(medoid_better(t_top, 5, t_top - 1, 0) && !medoid_better(t_top - 1, 0, t_top, 5) && medoid_better(0, 7, -1, 0) && !medoid_better(t_bottom, 0, 0, 7),
        "one unit of T decides");
  CHECK(medoid_better(t_top, 3, t_top, 4) && !medoid_better(t_top, 4, t_top, 3) && !medoid_better(t_top, 3, t_top, 3), "a tie goes to the smaller number");

  long checked = 0;
  for (int trial = 0; trial < 200000; trial++) {
    LinkCand a, b;
    a.n = 1 + (long long)(rnd() % (uint64_t)pairs); b.n = trial % 3 ? 1 + (long long)(rnd() % (uint64_t)pairs) : a.n + (long long)(rnd() % 3);
    const long long w = (long long)(rnd() % (uint64_t)(LINK_MAX_W + 1));
    a.s = w * a.n; b.s = w * b.n;
    if (trial % 2) {
      const long long da = (long long)(rnd() % 3), db = (long long)(rnd() % 3);
      if (da <= a.s) a.s -= da;
      if (db <= b.s) b.s -= db;
    }
    a.lo = (int32_t)(rnd() % 5); a.hi = a.lo + 1 + (int32_t)(rnd() % 5); b.lo = (int32_t)(rnd() % 5); b.hi = b.lo + 1 + (int32_t)(rnd() % 5);
    int want = by_division(a, b);
    if (want == 2) want = a.lo != b.lo ? (a.lo < b.lo) : a.hi != b.hi ? (a.hi < b.hi) : 2;
    CHECK(link_order(a, b) == want, "trial %d: %lld / %lld against %lld / %lld", trial, a.s, a.n, b.s, b.n);
    CHECK(link_order(b, a) == (want == 2 ? 2 : 1 - want), "trial %d: not antisymmetric", trial);
    checked++;
  }
  printf("%ld random pairs of candidates ordered\n", checked);
  if (failures) { printf("%d checks FAILED\n", failures); return 1; }
  printf("all checks passed\n");
  return 0;
}
