// fa_link.h -- the integer arithmetic of average-linkage clustering (fa_table_linkage, fa_linkage.hip.h): plain C++, no HIP.
// The kernels and fa_debug_linkage_order call the same functions, so the exactness of the order is testable without a GPU.
// The last part holds the same for the medoids of given clusters (fa_table_medoids, fa_medoid.hip.h, fa_debug_medoid_better).
//
// Identities are fixed point, 20 fractional bits: w = rint(identity * 2^20), ties to even.  A float32 at or above 16 is a
// multiple of 2^-19, so the float64 mean of two of them is a multiple of 2^-20 and the conversion is exact for everything
// FastANI reports.  A candidate is a pair of clusters {A, B} with
//     s = sum of w over the present pairs between them + qm * (|A||B| - their number),     n = |A||B|,
// and its average is s / n.  With at most 2^18 genomes n <= 2^34 and, w being at most 128 * 2^20, s <= 2^61: the cross
// products that compare two averages stay below 2^96 and are taken in 128 bits.  No floating point decides an order.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FA_LINK_FN __host__ __device__ inline
#else
#define FA_LINK_FN inline
#endif

namespace fa {

constexpr int32_t LINK_MAX_GENOMES = 1 << 18;
constexpr double LINK_SCALE = 1048576.0;                   // 2^20
constexpr double LINK_MAX_IDENTITY = 128.0;
constexpr long long LINK_MAX_W = 128LL << 20;

// the sum over the present pairs between two clusters and their number: what a merge adds up
struct LinkSum {
  long long w, c;
};
struct LinkSumPlus {
  FA_LINK_FN LinkSum operator()(const LinkSum &x, const LinkSum &y) const { return LinkSum{x.w + y.w, x.c + y.c}; }
};

// a candidate under the order of step 4; n == 0 stands for "none" and comes after every candidate
struct LinkCand {
  long long s, n;
  int32_t lo, hi;
};

// whether an identity can be converted at all (false for NaN)
FA_LINK_FN bool link_identity_ok(double identity) { return identity >= 0.0 && identity <= LINK_MAX_IDENTITY; }

// rint(x * 2^20), ties to even; x in [0, 2^40]
FA_LINK_FN long long link_fixed(double x) { return (long long)rint(x * LINK_SCALE); }

FA_LINK_FN long long link_s(const LinkSum &sum, long long n, long long qm) { return sum.w + qm * (n - sum.c); }

// s / n >= qc
FA_LINK_FN bool link_passes(long long s, long long n, long long qc) { return s >= qc * n; }

// 1: a comes before b; 0: b comes before a; 2: they are the same candidate.  Larger average first, compared as
// a.s * b.n against b.s * a.n in 128 bits; ties to the smaller lo, then to the smaller hi.  s >= 0, n >= 1.
FA_LINK_FN int link_order(const LinkCand &a, const LinkCand &b) {
  const unsigned __int128 x = (unsigned __int128)(unsigned long long)a.s * (unsigned long long)b.n;
  const unsigned __int128 y = (unsigned __int128)(unsigned long long)b.s * (unsigned long long)a.n;
  if (x != y) return x > y ? 1 : 0;
  if (a.lo != b.lo) return a.lo < b.lo ? 1 : 0;
  if (a.hi != b.hi) return a.hi < b.hi ? 1 : 0;
  return 2;
}

// the same with "none" on either side: whether b replaces a as the best so far
FA_LINK_FN bool link_better(const LinkCand &b, const LinkCand &a) {
  if (b.n == 0) return false;
  if (a.n == 0) return true;
  return link_order(b, a) == 1;
}

// ---- the merge list (fa_table_dendrogram, fa_dendrogram_cut): a merge {lo, hi, size_lo, size_hi, s, present} is the
// candidate {s, size_lo * size_hi, lo, hi} the walk merged, and the list is sorted under link_order
// whether a record can be a merge of a table of n_genomes <= LINK_MAX_GENOMES genomes: with it size_lo * size_hi <= 2^34, so
// link_passes does not overflow for any cut-off the drivers pass on (qc <= LINK_MAX_W + 1)
FA_LINK_FN bool link_merge_ok(int32_t lo, int32_t hi, int32_t size_lo, int32_t size_hi, long long s, long long present,
                              int32_t n_genomes) {
  return lo >= 0 && lo < hi && hi < n_genomes && size_lo >= 1 && size_hi >= 1 && (long long)size_lo + (long long)size_hi <= (long long)n_genomes &&
         s >= 0 && present >= 1;
}

FA_LINK_FN LinkCand link_merge_cand(int32_t lo, int32_t hi, int32_t size_lo, int32_t size_hi, long long s) {
  return LinkCand{s, (long long)size_lo * (long long)size_hi, lo, hi};
}

// the fixed-point cut-off of a float parameter, as fa_table_linkage forms qc: no weight exceeds LINK_MAX_W, so a cut-off above
// it merges nothing whatever its value, and neither does the clamped one.  value >= 0 (not NaN)
FA_LINK_FN long long link_cutoff(float value) {
  const double d = rint((double)value * LINK_SCALE);
  return d < (double)(LINK_MAX_W + 1) ? (long long)d : LINK_MAX_W + 1;
}

// ---- centrality and medoids (fa_table_medoids, fa_medoid.hip.h).  A member g of a cluster of m genomes has
//     S = sum of w over its present pairs inside the cluster + qm * (m - 1 - their number)           (< 2^46)
//     T = S + qb * (m - 1),   qb = rint(bonus * 2^20), |bonus| <= 32768                             (|T| < 2^54)
// so T / (m - 1) is "mean identity to the others + bonus", and within one cluster (one m) the order of T is its order.
constexpr double MEDOID_MAX_BONUS = 32768.0;

// whether a bonus can be converted at all (false for NaN)
FA_LINK_FN bool medoid_bonus_ok(double bonus) { return bonus >= -MEDOID_MAX_BONUS && bonus <= MEDOID_MAX_BONUS; }

// rint(bonus * 2^20), ties to even; medoid_bonus_ok(bonus)
FA_LINK_FN long long medoid_qb(double bonus) { return (long long)rint(bonus * LINK_SCALE); }

// the centrality sum of a member: `w` and `c` are the sum and the number of its present pairs inside its cluster of m >= 1
FA_LINK_FN long long medoid_s(long long w, long long c, long long m, long long qm) { return w + qm * (m - 1 - c); }

FA_LINK_FN long long medoid_t(long long s, long long qb, long long m) { return s + qb * (m - 1); }

// T as an unsigned key of the same order (the sign bit flipped): what a 64-bit atomicMax can decide.  Never 0 for |T| < 2^63
FA_LINK_FN unsigned long long medoid_key(long long t) { return (unsigned long long)t ^ 0x8000000000000000ULL; }

// whether member b with T = tb replaces member a with T = ta as the medoid: the larger T, ties to the smaller genome number.
// The kernels decide the same relation in two order-independent steps: the largest medoid_key of the cluster, then the
// smallest genome number among the members that reach it
FA_LINK_FN bool medoid_better(long long tb, int32_t b, long long ta, int32_t a) {
  const unsigned long long kb = medoid_key(tb), ka = medoid_key(ta);
  return kb != ka ? kb > ka : b < a;
}

}  // namespace fa
