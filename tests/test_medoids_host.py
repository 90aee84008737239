"""The host side of centrality and medoids (fa_table_medoids, include/fastani_hip.h) -- no GPU: the symbol, the arithmetic of
csrc/fa_link.h as `fa_debug_medoid_better` returns it -- the `__host__ __device__` functions the kernels call -- against Python
integers, every argument check that comes before any device work, and what a valid call does without a device."""
import ctypes as C

import numpy as np
import pytest

import table_medoids as tm
from conftest import has_gpu
from pyfastani_amd import _lib, clusters, outputs, sharding
from pyfastani_amd._lib import FA_ERR_INVALID, FA_ERR_NO_DEVICE, FA_ERR_UNSUPPORTED, FA_OK, lib

CASE = tm.cases()["random_65_05_three_values"]
POISON = -7


def test_the_symbols():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("fa_table_medoids", "fa_debug_medoid_better"):
        assert name in _lib.SIGNATURES and hasattr(raw, name)
    assert len(_lib.SIGNATURES["fa_table_medoids"][1]) == 18
    assert clusters.Medoids._fields == ("labels", "identity", "centrality", "size")
    assert callable(clusters.medoids) and callable(sharding.ResidentHitTable.medoids)


def better(bonus_b, s_b, b, bonus_a, s_a, a, m):
    t, out = (C.c_int64 * 2)(-1, -1), C.c_int32(-1)
    code = lib.fa_debug_medoid_better(bonus_b, s_b, b, bonus_a, s_a, a, m, t, C.byref(out))
    return code, list(t), out.value


def test_the_arithmetic_of_the_medoid_against_python_integers():
    g = np.random.default_rng(11)
    top = (1 << 46) - 1
    values = [0, 1, 2, top, top - 1, 97 << 20, (97 << 20) + 1]
    bonuses = [0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 2.0 ** -21, 3 * 2.0 ** -21, 32768.0, -32768.0, 0.1, 99.99, -5.25]
    sizes = [1, 2, 3, 65, 1 << 18]
    for _ in range(4000):
        s_b, s_a = (int(g.choice(values)) if g.random() < 0.7 else int(g.integers(0, top)) for _ in range(2))
        bonus_b, bonus_a = (float(g.choice(bonuses)) if g.random() < 0.7 else float(g.uniform(-32768, 32768)) for _ in range(2))
        m, b, a = int(g.choice(sizes)), int(g.integers(0, 1 << 18)), int(g.integers(0, 1 << 18))
        code, t, out = better(bonus_b, s_b, b, bonus_a, s_a, a, m)
        assert code == FA_OK, _lib.last_error()
        want = [s_b + tm.fixed64(bonus_b) * (m - 1), s_a + tm.fixed64(bonus_a) * (m - 1)]
        assert t == want and abs(t[0]) < 1 << 54
        assert out == int((want[0], -b) > (want[1], -a))
    # ties to even in the bonus; the smaller number wins a tie; a negative T orders below a positive one
    assert better(2.0 ** -21, 0, 1, 0.0, 0, 0, 2)[1] == [0, 0] and better(3 * 2.0 ** -21, 0, 1, 0.0, 0, 0, 2)[1] == [2, 0]
    assert better(0.0, 5, 3, 0.0, 5, 4, 7)[2] == 1 and better(0.0, 5, 4, 0.0, 5, 3, 7)[2] == 0 and better(0.0, 5, 3, 0.0, 5, 3, 7)[2] == 0
    assert better(-1.0, 0, 0, 0.0, 0, 9, 3) == (FA_OK, [-(2 << 20), 0], 0)
    assert better(-32768.0, 0, 0, -32768.0, 1, 9, 1 << 18)[2] == 0
    nan = float("nan")
    for bad in ((nan, 0, 0, 0.0, 0, 1, 2), (0.0, 0, 0, 32768.5, 0, 1, 2), (0.0, -1, 0, 0.0, 0, 1, 2), (0.0, 0, 0, 0.0, 1 << 46, 1, 2),
                (0.0, 0, -1, 0.0, 0, 1, 2), (0.0, 0, 0, 0.0, 0, 1, 0), (0.0, 0, 0, 0.0, 0, 1, (1 << 18) + 1)):
        assert better(*bad) == (FA_ERR_INVALID, [-1, -1], -1), bad
    assert lib.fa_debug_medoid_better(0.0, 0, 0, 0.0, 0, 1, 2, None, None) == FA_ERR_INVALID


def call(case=CASE, missing=0.0, params=True, n=None, lengths=True, fragment_length=None, n_rows=None, rows=True, labels=True, n_sets=1,
         bonus=None, label_values=None):
    """fa_table_medoids on host pointers: (code, the four outputs, n_clusters, stats), the outputs starting as poison"""
    n = case["n"] if n is None else n
    p = _lib.TableParams(case["min_fraction"], case["fragment_length"] if fragment_length is None else fragment_length, float("nan"), 0)
    qlen = np.resize(case["query_lengths"], max(n, 1)).astype(np.uint64)
    room = max(n, 1) * max(n_sets, 1)
    h_labels = np.zeros(room, dtype=np.int32) if label_values is None else np.ascontiguousarray(label_values, dtype=np.int32)
    out = [np.full(room, POISON, dtype=kind) for kind in (np.int32, np.float64, np.int64, np.int32)]
    n_clusters, stats = np.full(max(n_sets, 1), -1, dtype=np.int32), (C.c_int64 * 4)(*[-1] * 4)
    bonus = None if bonus is None else np.ascontiguousarray(np.resize(np.asarray(bonus, dtype=np.float64), max(n, 1)))
    code = lib.fa_table_medoids(C.c_void_p(case["rows"].ctypes.data) if rows else None, len(case["rows"]) if n_rows is None else n_rows, 0, n,
                                C.c_void_p(qlen.ctypes.data) if lengths else None, C.c_void_p(qlen.ctypes.data) if lengths else None,
                                C.byref(p) if params else None, missing, C.c_void_p(h_labels.ctypes.data) if labels else None, n_sets,
                                C.c_void_p(bonus.ctypes.data) if bonus is not None else None, *[C.c_void_p(x.ctypes.data) for x in out], 0,
                                C.c_void_p(n_clusters.ctypes.data), stats)
    return code, out, n_clusters, list(stats)


def untouched(got):
    code, out, n_clusters, stats = got
    return all(np.all(x == POISON) for x in out) and np.all(n_clusters == -1) and stats == [-1] * 4


def test_bad_arguments_are_reported_before_any_device_work():
    nan, n = float("nan"), CASE["n"]
    out_of_range, not_its_own = np.zeros((3, n), dtype=np.int32), np.zeros((3, n), dtype=np.int32)
    out_of_range[2, n - 1] = n                                       # in the last set only
    not_its_own[1, 5], not_its_own[1, 7] = 7, 5                      # 5 -> 7 -> 5: neither labels itself
    invalid = [dict(params=False), dict(missing=-0.5), dict(missing=nan), dict(missing=128.5), dict(missing=float("inf")), dict(lengths=False),
               dict(fragment_length=0), dict(n=-1), dict(n_rows=-1), dict(rows=False), dict(n_sets=0), dict(n_sets=-1), dict(labels=False),
               dict(bonus=[0.0, nan]), dict(bonus=[32768.5]), dict(bonus=[0.0, 0.0, -float("inf")]),
               dict(n_sets=3, label_values=out_of_range), dict(n_sets=3, label_values=not_its_own),
               dict(label_values=np.full(n, -1, dtype=np.int32))]
    for kw in invalid:
        got = call(**kw)
        assert got[0] == FA_ERR_INVALID, (kw, got[0], _lib.last_error())
        assert untouched(got), kw
    got = call(n=2 ** 18 + 1)
    assert got[0] == FA_ERR_UNSUPPORTED and b"2^18" in lib.fa_last_error() and untouched(got)
    # 2^31 labels: refused before they are read
    p, qlen = _lib.TableParams(0.2, 3000, 0.0, 0), np.ones(2 ** 18, dtype=np.uint64)
    code = lib.fa_table_medoids(None, 0, 0, 2 ** 18, C.c_void_p(qlen.ctypes.data), C.c_void_p(qlen.ctypes.data), C.byref(p), 0.0,
                                C.c_void_p(qlen.ctypes.data), 2 ** 13, None, None, None, None, None, 0, None, None)
    assert code == FA_ERR_UNSUPPORTED and b"2^31" in lib.fa_last_error()


def test_the_python_mappings():
    n = CASE["n"]
    args = (CASE["rows"], CASE["query_lengths"], CASE["reference_lengths"], CASE["fragment_length"])
    zeros = np.zeros(n, dtype=np.int32)
    bad = zeros.copy()
    bad[3] = n
    for kw, match in ((dict(labels=zeros, missing=float("nan")), "missing"), (dict(labels=zeros, missing=129.0), "missing"),
                      (dict(labels=zeros, bonus=np.full(n, np.nan)), "bonus"), (dict(labels=bad), "label"),
                      (dict(labels=zeros[:-1]), "labels"), (dict(labels=np.zeros((0, n), dtype=np.int32)), "labels"),
                      (dict(labels=zeros.astype(np.float64)), "labels"), (dict(labels=zeros, bonus=np.zeros(n + 1)), "bonus")):
        with pytest.raises(ValueError, match=match):
            clusters.medoids(*args, **kw)
    import torch
    with pytest.raises(ValueError, match="labels"):
        clusters.medoids(*args, labels=torch.zeros(n, dtype=torch.int32))              # a tensor with host rows
    ones = np.ones(2 ** 18 + 1, dtype=np.uint64)
    with pytest.raises(NotImplementedError, match="2\\^18"):
        clusters.medoids(CASE["rows"], ones, ones, 3000, np.zeros(2 ** 18 + 1, dtype=np.int32))


@pytest.mark.skipif(has_gpu(), reason="CPU-only behaviour")
def test_without_a_device_a_valid_call_fails_loudly():
    got = call()
    assert got[0] == FA_ERR_NO_DEVICE and b"no HIP device" in lib.fa_last_error() and untouched(got)
    assert call(n_sets=3, bonus=[1.0, -2.0], missing=128.0)[0] == FA_ERR_NO_DEVICE
    got = call(tm.cases()["no_rows"], n=2 ** 18)                    # the largest supported number of genomes
    assert got[0] == FA_ERR_NO_DEVICE and untouched(got)
    with pytest.raises(RuntimeError, match="no HIP device"):
        clusters.medoids(CASE["rows"], CASE["query_lengths"], CASE["reference_lengths"], CASE["fragment_length"],
                         np.zeros(CASE["n"], dtype=np.int32))


def test_a_nan_identity_is_written_as_nan(tmp_path):
    outputs.write_representatives(tmp_path / "m.tsv", ["a", "b", "c"], np.array([0, 0, 0], dtype=np.int32), np.array([100.0, 97.5, tm.NAN]))
    assert (tmp_path / "m.tsv").read_text() == "a\ta\t100\nb\ta\t97.5\nc\ta\tnan\n"
