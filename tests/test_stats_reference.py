"""The parameter statistics against Boost.Math, the library the reference's skch::Stat calls.

fa_stats.h stands in for boost::math::quantile(complement(binomial(s, p), q)) and for the binomial tail with a
double-precision summation of lgamma pmf terms, and the CPU oracle computes them the same way: the oracle comparison of
the GPU tests cannot catch a wrong quantile.  SciPy's ``binom.isf`` / ``binom.sf`` are built on Boost.Math, so here the
C ABI (fa_mapping_identity, fa_estimate_minimum_hits_relaxed, fa_recommended_window_size) is compared bit for bit with a
model that takes j2md / md2j exactly as fa_stats.h documents them (float32 where the C++ is float, double where it is
double, the same libm functions) and its quantile and tail from SciPy.  The identity LUT, the pass table and min_hits
of every kernel are built by the same functions (StatTables::extend), and StatTables::extend walks on the upper bound being
monotone in the shared count -- asserted here for every sketch size checked (from c = 1 on; see check_sketch_size)."""
import ctypes as C
import ctypes.util
import math

import numpy as np
import pytest

from pyfastani_amd._lib import lib, check

stats = pytest.importorskip("scipy.stats")

f32 = np.float32
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]
Q2 = (1.0 - float(f32(0.9))) / 2.0          # kConfidence is the float 0.9f: q2 = (1 - (double)ci) / 2


def j2md(j, k):
    # float r = (-1.0 / k) * log(2.0 * j / (1 + j)), (1 + j) in float
    j = f32(j)
    if j == 0:
        return f32(1.0)
    if j == 1:
        return f32(0.0)
    return f32((-1.0 / k) * math.log(2.0 * float(j) / float(f32(1) + j)))


def md2j(d, k):
    # float r = 1.0 / (2.0 * exp(k * d) - 1.0), k * d in float, exp the float overload
    kd = f32(f32(k) * f32(d))
    return f32(1.0 / (2.0 * float(_libm.expf(float(kd))) - 1.0))


def boost_quantile(s, p):
    return int(stats.binom.isf(Q2, s, p))


def model_identity(c, s, k):
    md = j2md(f32(1.0 * c / s), k)
    x = boost_quantile(s, float(md2j(md, k)))
    lo = j2md(f32(x) / f32(s), k)
    return f32(100) * (f32(1) - md), f32(100) * (f32(1) - lo)


def model_min_hits(s, k, pid):
    pid = f32(pid)
    first = int(math.ceil(1.0 * s * float(md2j(f32(1.0 - float(pid) / 100.0), k))))
    relaxed = first
    for i in range(first, -1, -1):
        d = j2md(f32(1.0 * i / s), k)
        lo = j2md(f32(boost_quantile(s, float(md2j(d, k)))) / f32(s), k)
        if f32(100.0 * (1.0 - float(lo))) >= pid:
            relaxed = i
        else:
            break
    return relaxed


def model_window(p_value, k, pid, frag, ref_size=5_000_000):
    px = 1.0 / (1.0 + math.pow(4.0, k) / frag)
    r = px * px / (px + px - px * px)
    for s in [1, 2, 5] + list(range(10, frag, 10)):
        x = model_min_hits(s, k, pid)
        tail = 1.0 if x == 0 else float(stats.binom.sf(x - 1, s, r))
        if ref_size * tail <= p_value:
            return min(max(int(2.0 * frag / s), 1), frag)
    return -1


def abi_identity(c, s, k):
    ident, upper = C.c_float(), C.c_float()
    check(lib.fa_mapping_identity(c, s, k, C.byref(ident), C.byref(upper)))
    return f32(ident.value), f32(upper.value)


def abi_min_hits(s, k, pid):
    h = C.c_int()
    check(lib.fa_estimate_minimum_hits_relaxed(s, k, pid, C.byref(h)))
    return h.value


def abi_window(p_value, k, pid, frag, ref_size=5_000_000):
    w = C.c_int()
    check(lib.fa_recommended_window_size(p_value, k, 4, pid, frag, ref_size, C.byref(w)))
    return w.value


def check_sketch_size(s, k, cs):
    """identity and upper bound bit for bit at every shared count in `cs` (ascending); the upper bound monotone over them
    from c = 1 on.  c = 0 is the one exception: j2md(0) is defined as 1, while j2md(1 / s) exceeds 1 once 2 / (s + 1) < e^-k
    (k <= 7 in protein mode, s of a few hundred and more), so upper(0) > upper(1) there.  pass_shared (the walk of
    StatTables::extend) then says "0 fails" although upper(0) >= pid for pid in (upper(1), upper(0)].  At the 0.9 interval
    checked here the minimum hit count is at least 2 in exactly that range (asserted below); that alone does not keep a locus
    from sharing 0 records in its best window, so the library refuses such parameters instead of relying on it
    (fa_stats.h: stat_zero_passes_alone; tests/test_rules_domain_inputs.py checks the refusal at every interval)."""
    ups = {}
    for c in cs:
        got, want = abi_identity(c, s, k), model_identity(c, s, k)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (s, c, k, got, want)
        ups[c] = got[1]
    rising = [ups[c] for c in sorted(ups) if c >= 1]
    assert all(a <= b for a, b in zip(rising, rising[1:])), f"upper bound falls with c at s={s} k={k}"
    if 0 in ups and 1 in ups and ups[0] > ups[1]:
        assert k <= 7, (s, k)
        for pid in (ups[0], np.nextafter(ups[1], f32(np.inf))):
            assert abi_min_hits(s, k, float(pid)) >= 2, (s, k, pid)


def sampled_sizes(lo, hi, n, seed):
    g = np.random.default_rng(seed)
    return sorted(set(g.integers(lo, hi + 1, n).tolist()) | {hi})


@pytest.mark.parametrize("k", [14, 16, 21])
def test_identity_and_upper_bound_every_shared_count_to_600(k):
    for s in range(1, 601):
        check_sketch_size(s, k, range(s + 1))


@pytest.mark.parametrize("k", [14, 16, 21])
def test_identity_and_upper_bound_sampled_to_3400(k):
    for s in sampled_sizes(601, 3400, 10, 7 + k):
        check_sketch_size(s, k, range(s + 1))


@pytest.mark.parametrize("k", [5, 7])
def test_identity_and_upper_bound_protein_to_12000(k):
    # protein mode: w = 1, a fragment of 12 000 residues keeps up to ~12 000 minimizers
    g = np.random.default_rng(k)
    for s in sampled_sizes(1, 12_000, 12, 100 + k):
        cs = sorted(set(g.integers(0, s + 1, 150).tolist()) | {0, s // 2, s - 1 if s > 1 else 0, s})
        check_sketch_size(s, k, cs)


@pytest.mark.parametrize("pid", [64.5, 68.0, 70.0, 80.0, 90.0, 95.0, 96.0, 99.0, 100.0])
@pytest.mark.parametrize("k", [14, 16, 21])
def test_minimum_hits_relaxed(k, pid):
    sizes = list(range(1, 301)) + sampled_sizes(301, 3400, 25, int(pid * 10) + k)
    for s in sizes:
        assert abi_min_hits(s, k, pid) == model_min_hits(s, k, pid), (s, k, pid)


# (p_value, k, percentage_identity, fragment_length, reference_size) -> the recommended window
WINDOWS = [
    (1e-3, 16, 64.5, 3000, 5_000_000, 2), (1e-3, 16, 67.0, 3000, 5_000_000, 3), (1e-3, 16, 69.0, 3000, 5_000_000, 4),
    (1e-3, 16, 80.0, 3000, 5_000_000, 24), (1e-3, 16, 96.0, 3000, 5_000_000, 600), (1e-3, 16, 99.0, 3000, 5_000_000, 1200),
    (1e-3, 16, 100.0, 3000, 5_000_000, 1200),
    (1e-3, 14, 68.5, 1000, 5_000_000, 2), (1e-3, 14, 95.0, 1000, 5_000_000, 200), (1e-3, 14, 98.0, 1000, 5_000_000, 400),
    (1e-3, 21, 68.0, 5000, 5_000_000, 2), (1e-3, 21, 70.0, 5000, 5_000_000, 3), (1e-3, 21, 97.0, 5000, 5_000_000, 1000),
    (1e-3, 21, 99.0, 5000, 5_000_000, 2000),
    (1e-3, 16, 96.0, 500, 5_000_000, 100), (1e-3, 16, 99.0, 500, 5_000_000, 200),
    (1e-1, 16, 80.0, 3000, 5_000_000, 40), (1e-8, 16, 80.0, 3000, 5_000_000, 20), (1e-12, 16, 80.0, 3000, 5_000_000, 15),
]


@pytest.mark.parametrize("p_value,k,pid,frag,ref_size,w", WINDOWS)
def test_recommended_window_sizes(p_value, k, pid, frag, ref_size, w):
    assert abi_window(p_value, k, pid, frag, ref_size) == w
    assert model_window(p_value, k, pid, frag, ref_size) == w


def test_reference_size_moves_the_window():
    for ref_size in (10_000, 5_000_000, 3_000_000_000):
        assert abi_window(1e-3, 16, 80.0, 3000, ref_size) == model_window(1e-3, 16, 80.0, 3000, ref_size)
    assert abi_window(1e-3, 16, 80.0, 3000, 10_000) != abi_window(1e-3, 16, 80.0, 3000, 3_000_000_000)
