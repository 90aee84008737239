"""The host side of average-linkage clustering (fa_table_linkage, include/fastani_hip.h) -- no GPU: the order of step 4 as
`fa_debug_linkage_order` returns it -- the `__host__ __device__` comparator of csrc/fa_link.h that the kernels call -- against
Python integers where float64 cannot tell the candidates apart, and the checks of step 7 that come before any device work."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import table_linkage as tl
from conftest import has_gpu
from pyfastani_amd import _lib, clusters
from pyfastani_amd._lib import FA_ERR_INVALID, FA_ERR_NO_DEVICE, FA_ERR_UNSUPPORTED, FA_OK, lib

W96 = 96 * 2 ** 20


def library_order(a, b):
    first = C.c_int(-1)
    code = lib.fa_debug_linkage_order((C.c_int64 * 4)(*a), (C.c_int64 * 4)(*b), C.byref(first))
    assert code == FA_OK, _lib.last_error()
    return first.value


def integer_order(a, b):
    """step 4 in Python integers: 1 when a comes first, 0 when b does, 2 when they are equal"""
    x, y = a[0] * b[1], b[0] * a[1]
    if x != y:
        return 1 if x > y else 0
    if a[2:] != b[2:]:
        return 1 if a[2:] < b[2:] else 0
    return 2


def candidates():
    """pairs of candidates (S, |A||B|, lo, hi), each labelled by what it is there for"""
    out = {}
    # averages that differ by 1 / (n1 * n2) of a fixed-point unit only
    out["one_part_in_n1_n2"] = ((22500 * W96 + 22499, 22500, 3, 5), (22499 * W96 + 22498, 22499, 1, 2))
    out["the_same_average_other_sizes"] = ((22500 * W96, 22500, 3, 5), (22499 * W96, 22499, 1, 2))
    # S near 2^61 over |A||B| near 2^34: the cross products are near 2^95
    big_n, other_n = 2 ** 34 - 3, 2 ** 34 - 5
    out["products_beyond_64_bits"] = ((2 ** 27 * big_n - 1, big_n, 0, 1), (2 ** 27 * other_n - 1, other_n, 2, 3))
    out["products_beyond_64_bits_tie"] = ((2 ** 27 * big_n, big_n, 4, 9), (2 ** 27 * other_n, other_n, 2, 30))
    out["low_words_decide"] = ((2 ** 61 - 1, 2 ** 34, 0, 1), (2 ** 61 - 2 ** 27 - 1, 2 ** 34 - 1, 0, 2))
    # the largest arguments the helper takes
    out["largest_arguments"] = ((2 ** 63 - 1, 2 ** 63 - 1, 0, 1), (2 ** 63 - 2, 2 ** 63 - 1, 0, 2))
    # exact ties: lo decides, then hi
    out["tie_lo_decides"] = ((3 * W96, 3, 1, 9), (2 * W96, 2, 2, 3))
    out["tie_hi_decides"] = ((3 * W96, 3, 1, 9), (2 * W96, 2, 1, 4))
    out["equal"] = ((6 * W96, 6, 1, 4), (6 * W96, 6, 1, 4))
    out["zero_sums"] = ((0, 4, 2, 3), (0, 9, 1, 7))
    out["zero_against_one"] = ((0, 1, 0, 1), (1, 2 ** 34, 5, 6))
    return out


@pytest.mark.parametrize("name", sorted(candidates()))
def test_the_order_is_exact(name):
    a, b = candidates()[name]
    want = integer_order(a, b)
    assert library_order(a, b) == want
    assert library_order(b, a) == {0: 1, 1: 0, 2: 2}[want]
    assert library_order(a, a) == 2 and library_order(b, b) == 2
    # the second definition: rationals
    fa, fb = Fraction(a[0], a[1]), Fraction(b[0], b[1])
    assert want == (1 if fa > fb else 0 if fa < fb else integer_order((0, 1) + a[2:], (0, 1) + b[2:]))


def test_the_cases_are_what_they_claim():
    c = candidates()
    a, b = c["one_part_in_n1_n2"]
    assert Fraction(a[0], a[1]) - Fraction(b[0], b[1]) == Fraction(1, 22500 * 22499)
    assert a[0] / a[1] == b[0] / b[1]                                # float64 cannot tell them apart
    assert integer_order(a, b) == 1 and a[2:] > b[2:]                # ... and the tie rule would say the opposite
    for name in ("products_beyond_64_bits", "products_beyond_64_bits_tie", "low_words_decide"):
        a, b = c[name]
        assert a[0] * b[1] > 2 ** 64 and b[0] * a[1] > 2 ** 64 and max(a[0], b[0]) < 2 ** 61 + 1 and a[1] >= 2 ** 33
    a, b = c["products_beyond_64_bits"]
    assert a[0] / a[1] == b[0] / b[1] and integer_order(a, b) == 1   # float64 sees a tie, and lo would also say "a": so
    assert integer_order(b[:2] + a[2:], a[:2] + b[2:]) == 0          # swap the labels and the exact order still wins
    assert library_order(b[:2] + a[2:], a[:2] + b[2:]) == 0
    a, b = c["low_words_decide"]
    assert (a[0] * b[1]) >> 64 == (b[0] * a[1]) >> 64                # equal high words


def test_random_candidates_against_integers():
    g = np.random.default_rng(4)
    for _ in range(2000):
        sizes = [int(v) for v in g.integers(1, 2 ** 17, 4)]
        n1, n2 = sizes[0] * sizes[1], sizes[2] * sizes[3]
        w = int(g.integers(0, 128 * 2 ** 20 + 1))
        s1 = min(w * n1 + int(g.integers(-2, 3)), 128 * 2 ** 20 * n1)
        s2 = min(w * n2 + int(g.integers(-2, 3)), 128 * 2 ** 20 * n2)
        a = (max(s1, 0), n1, int(g.integers(0, 4)), int(g.integers(4, 8)))
        b = (max(s2, 0), n2, int(g.integers(0, 4)), int(g.integers(4, 8)))
        assert library_order(a, b) == integer_order(a, b), (a, b)


def test_the_helper_refuses_what_is_no_candidate():
    first = C.c_int(-1)
    good = (C.c_int64 * 4)(5, 1, 0, 1)
    for bad in ((-1, 1, 0, 1), (5, 0, 0, 1), (5, -3, 0, 1), (5, 1, -1, 1), (5, 1, 0, 2 ** 31)):
        assert lib.fa_debug_linkage_order((C.c_int64 * 4)(*bad), good, C.byref(first)) == FA_ERR_INVALID
        assert lib.fa_debug_linkage_order(good, (C.c_int64 * 4)(*bad), C.byref(first)) == FA_ERR_INVALID
    assert lib.fa_debug_linkage_order(None, good, C.byref(first)) == FA_ERR_INVALID
    assert lib.fa_debug_linkage_order(good, None, C.byref(first)) == FA_ERR_INVALID
    assert lib.fa_debug_linkage_order(good, good, None) == FA_ERR_INVALID
    assert first.value == -1


def call(case, min_identity=95.0, missing=0.0, params=True, n=None, lengths=True, fragment_length=None, n_rows=None, rows=True):
    """fa_table_linkage on host pointers: (code, labels, n_clusters, stats), the outputs starting as poison"""
    n = case["n"] if n is None else n
    p = _lib.TableParams(case["min_fraction"], case["fragment_length"] if fragment_length is None else fragment_length, min_identity, 0)
    qlen = np.resize(case["query_lengths"], max(n, 1)).astype(np.uint64)
    labels, count, stats = np.full(max(n, 1), -7, dtype=np.int32), C.c_int32(-1), (C.c_int64 * 5)(*[-1] * 5)
    code = lib.fa_table_linkage(C.c_void_p(case["rows"].ctypes.data) if rows else None, len(case["rows"]) if n_rows is None else n_rows, 0, n,
                                C.c_void_p(qlen.ctypes.data) if lengths else None, C.c_void_p(qlen.ctypes.data) if lengths else None,
                                C.byref(p) if params else None, missing, C.c_void_p(labels.ctypes.data), 0, C.byref(count), stats)
    return code, labels, count.value, list(stats)


def test_bad_arguments_are_reported_before_any_device_work():
    case = tl.cases()["random_65_05_three_values"]
    nan = float("nan")
    invalid = [dict(params=False), dict(min_identity=-1.0), dict(min_identity=nan), dict(missing=-0.5), dict(missing=nan),
               dict(missing=95.0), dict(missing=96.0), dict(min_identity=0.0, missing=0.0),
               dict(min_identity=float(np.nextafter(np.float32(1.0), np.float32(2))), missing=1.0),         # qm == qc after rounding
               dict(min_identity=float("inf"), missing=float("inf")), dict(lengths=False), dict(fragment_length=0), dict(n=-1),
               dict(n_rows=-1), dict(rows=False)]
    for kw in invalid:
        code, labels, count, stats = call(case, **kw)
        assert code == FA_ERR_INVALID, (kw, code, _lib.last_error())
        assert np.all(labels == -7) and count == -1 and stats == [-1] * 5
    assert tl.fixed(np.nextafter(np.float32(1.0), np.float32(2))) == tl.fixed(1.0)
    code, labels, count, stats = call(case, n=2 ** 18 + 1)
    assert code == FA_ERR_UNSUPPORTED and b"2^18" in lib.fa_last_error()
    assert np.all(labels == -7) and count == -1 and stats == [-1] * 5
    args = (case["rows"], case["query_lengths"], case["reference_lengths"], case["fragment_length"])
    for kw, match in ((dict(min_identity=-1.0), "min_identity"), (dict(missing=nan), "missing"), (dict(missing=95.0), "missing")):
        with pytest.raises(ValueError, match=match):
            clusters.average_linkage(*args, **kw)
    with pytest.raises(NotImplementedError, match="2\\^18"):
        clusters.average_linkage(case["rows"], np.ones(2 ** 18 + 1, dtype=np.uint64), np.ones(2 ** 18 + 1, dtype=np.uint64), 3000)


@pytest.mark.skipif(has_gpu(), reason="CPU-only behaviour")
def test_without_a_device_a_valid_call_fails_loudly():
    case = tl.cases()["random_65_05_three_values"]
    code, labels, count, stats = call(case)
    assert code == FA_ERR_NO_DEVICE and b"no HIP device" in lib.fa_last_error()
    assert np.all(labels == -7) and count == -1 and stats == [-1] * 5
    code, labels, count, stats = call(case, n=2 ** 18)               # the largest supported number of genomes
    assert code == FA_ERR_NO_DEVICE
    with pytest.raises(RuntimeError, match="no HIP device"):
        clusters.average_linkage(case["rows"], case["query_lengths"], case["reference_lengths"], case["fragment_length"])
