"""The genome-level screen on the device (fa_screen_signatures / fa_screen_pairs / fa_screen_groups, pyfastani_amd.screen)
against the plain restatement of tests/screen.py -- MI355X only.  Signatures, counts, records and labels are compared byte
for byte, the counters exactly.  The inputs are synthetic records and signatures but for the last test, which sketches
genomes (and maps only to show that the sketch is still whole)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import screen as sc
from pyfastani_amd import _lib, outputs, screen
from pyfastani_amd._lib import FA_ERR_INVALID, FA_OK, lib
from pyfastani_amd.screen import SCREEN_DTYPE

pytestmark = pytest.mark.gpu

SIGNATURE_CASES = sc.signature_cases()
PAIR_CASES = sc.pair_cases()
DEVICE = "cuda:0"


def to_device(array):
    """the bytes of a numpy array in HBM (uint32 has no torch dtype everywhere: the words travel as int32)"""
    flat = np.ascontiguousarray(array).reshape(-1)
    words = flat.view(np.int32) if flat.dtype.itemsize == 4 else flat.view(np.uint8)
    return torch.from_numpy(words.copy()).to(DEVICE)


def ptr(tensor):
    return C.c_void_p(tensor.data_ptr()) if tensor.numel() else None


# ---- signatures ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_signatures(name):
    return sc.restate_signatures(SIGNATURE_CASES[name])


def lib_signatures(case, s=None):
    """(status, sig bytes, count bytes): the outputs start as bytes 0xAB"""
    s = case["s"] if s is None else s
    n = len(case["sbf"])
    d_hash, d_seq = to_device(case["hash"]), to_device(case["seq_id"])
    d_sig = torch.full((n * max(s, 1) * 4,), 0xAB, dtype=torch.uint8, device=DEVICE)
    d_count = torch.full((n * 4,), 0xAB, dtype=torch.uint8, device=DEVICE)
    torch.cuda.synchronize()
    code = lib.fa_screen_signatures(ptr(d_hash), ptr(d_seq), len(case["hash"]), C.c_void_p(case["sbf"].ctypes.data), n, s,
                                    C.c_void_p(d_sig.data_ptr()), C.c_void_p(d_count.data_ptr()))
    return code, d_sig.cpu().numpy(), d_count.cpu().numpy()


@pytest.mark.parametrize("name", sorted(SIGNATURE_CASES))
def test_signatures_match_the_restatement(name):
    code, sig, count = lib_signatures(SIGNATURE_CASES[name])
    want_sig, want_count = expected_signatures(name)
    assert code == FA_OK, _lib.last_error()
    assert count.tobytes() == want_count.tobytes()
    assert sig.tobytes() == want_sig.tobytes()


def bad_records():
    case = SIGNATURE_CASES["mixed_s64"]
    out = {}
    descending = dict(case, seq_id=case["seq_id"].copy())
    descending["seq_id"][[200, 201]] = descending["seq_id"][[201, 200]] + np.array([1, 0], dtype=np.int32)
    out["contig_ids_descend"] = (descending, None)
    for label, value in (("contig_id_is_the_number_of_contigs", int(case["sbf"][-1])), ("contig_id_is_huge", 2 ** 31 - 1)):
        bad = dict(case, seq_id=case["seq_id"].copy())
        bad["seq_id"][-1] = value
        out[label] = (bad, None)
    negative = dict(case, seq_id=case["seq_id"].copy())
    negative["seq_id"][0] = -1
    out["contig_id_is_negative"] = (negative, None)
    down = dict(case, sbf=case["sbf"].copy())
    down["sbf"][3] = down["sbf"][2] - 1
    out["sbf_decreases"] = (down, None)
    out["size_is_zero"] = (case, 0)
    out["size_is_4097"] = (case, 4097)
    return out


@pytest.mark.parametrize("label", sorted(bad_records()))
def test_bad_records_are_invalid_and_leave_the_outputs_untouched(label):
    case, s = bad_records()[label]
    assert label != "contig_ids_descend" or np.any(np.diff(case["seq_id"]) < 0)
    code, sig, count = lib_signatures(case, s)
    assert code == FA_ERR_INVALID, (code, _lib.last_error())
    assert np.all(sig == 0xAB) and np.all(count == 0xAB)
    test_signatures_match_the_restatement("mixed_s64")                     # the process goes on


# ---- pairs -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_pairs(name):
    return sc.restate_pairs(PAIR_CASES[name])


def lib_pairs(case, pairs_device=False, cap=None, count_only=False, changes=None, **replaced):
    """(status, the whole record buffer as bytes, *n_pairs, stats); the buffer starts as bytes 0xAB, *n_pairs as -1 and
    stats as -1s.  ``changes(sig_a, count_a)`` edits copies of the first set; ``replaced`` replace s, jn, jd."""
    sig_a, count_a = case["sig_a"].copy(), case["count_a"].copy()
    if changes:
        changes(sig_a, count_a)
    d_sig_a, d_count_a = to_device(sig_a), to_device(count_a)
    same = case["sig_a"] is case["sig_b"]
    d_sig_b, d_count_b = (d_sig_a, d_count_a) if same else (to_device(case["sig_b"]), to_device(case["count_b"]))
    n_a, n_b = len(count_a), len(case["count_b"])
    total = n_a * (n_a - 1) // 2 if case["triangular"] else n_a * n_b
    cap = total + 3 if cap is None else cap
    n, stats = C.c_int64(-1), (C.c_int64 * 2)(-1, -1)
    head = (ptr(d_sig_a), ptr(d_count_a), n_a, ptr(d_sig_b), ptr(d_count_b), n_b, replaced.get("s", case["s"]),
            int(case["triangular"]), replaced.get("jn", case["jn"]), replaced.get("jd", case["jd"]))
    buffer = np.full(cap * 16, 0xAB, dtype=np.uint8)
    torch.cuda.synchronize()
    if pairs_device:
        d_buffer = torch.from_numpy(buffer.copy()).to(DEVICE)
        torch.cuda.synchronize()
        code = lib.fa_screen_pairs(*head, None if count_only else C.c_void_p(d_buffer.data_ptr()), cap, C.byref(n), 1, stats)
        buffer = d_buffer.cpu().numpy()
    else:
        code = lib.fa_screen_pairs(*head, None if count_only else C.c_void_p(buffer.ctypes.data), cap, C.byref(n), 0, stats)
    return code, buffer, n.value, tuple(stats)


def check_pairs(name, got, count_only=False):
    code, buffer, n, stats = got
    want, want_stats = expected_pairs(name)
    assert code == FA_OK, _lib.last_error()
    assert n == len(want) and stats == want_stats
    written = 0 if count_only else n * 16
    assert buffer[:written].tobytes() == want.tobytes()[:written]
    assert np.all(buffer[written:] == 0xAB)                                 # nothing is written behind the records


def untouched(got):
    return np.all(got[1] == 0xAB) and got[3] == (-1, -1)


@pytest.mark.parametrize("name", sorted(PAIR_CASES))
def test_pairs_match_the_restatement(name):
    check_pairs(name, lib_pairs(PAIR_CASES[name]))
    check_pairs(name, lib_pairs(PAIR_CASES[name], count_only=True), count_only=True)


@pytest.mark.parametrize("name", ["named_s1000_triangular", "tile_s1000_9_x_7", "three_mask_words_s8_triangular", "no_genomes"])
def test_host_and_device_records_agree(name):
    check_pairs(name, lib_pairs(PAIR_CASES[name], pairs_device=True))
    check_pairs(name, lib_pairs(PAIR_CASES[name], pairs_device=False))


@pytest.mark.parametrize("s", [8, 64, 1000, 4096])
def test_the_triangular_rows_are_the_rectangular_rows_above_the_diagonal(s):
    triangular = lib_pairs(PAIR_CASES[f"named_s{s}_triangular"])
    rectangular = lib_pairs(PAIR_CASES[f"named_s{s}_rectangular"])
    assert triangular[0] == rectangular[0] == FA_OK
    t = triangular[1][: triangular[2] * 16].view(SCREEN_DTYPE)
    r = rectangular[1][: rectangular[2] * 16].view(SCREEN_DTYPE)
    assert len(t) == 44 and len(r) == 96 and r[r["a"] < r["b"]].tobytes() == t.tobytes()


@pytest.mark.parametrize("pairs_device", [False, True])
def test_a_buffer_one_record_short_is_invalid(pairs_device):
    name = "several_tiles_s1000_triangular"
    n_records = len(expected_pairs(name)[0])
    assert n_records > 2
    got = lib_pairs(PAIR_CASES[name], pairs_device=pairs_device, cap=n_records - 1)
    assert got[0] == FA_ERR_INVALID and untouched(got), _lib.last_error()
    assert got[2] == n_records                                              # what the caller needs
    check_pairs(name, lib_pairs(PAIR_CASES[name], pairs_device=pairs_device, cap=n_records))


def set_count(g, value):
    def change(sig, count):
        count[g] = value
    return change


def break_order(g, at, equal):
    def change(sig, count):
        assert count[g] > at >= 1
        sig[g, at] = sig[g, at - 1] if equal else sig[g, at - 1] - 1
    return change


BAD_SIGNATURES = {
    "count_is_s_plus_one": set_count(2, 1001), "count_is_negative": set_count(17, -1), "count_is_huge": set_count(0, 2 ** 31 - 1),
    "a_signature_descends": break_order(5, 700, False), "a_signature_repeats_an_element": break_order(11, 1, True),
    "the_last_element_descends": break_order(17, 999, False),
}


@pytest.mark.parametrize("label", sorted(BAD_SIGNATURES))
@pytest.mark.parametrize("triangular", [True, False])
def test_bad_signatures_are_invalid_and_return_nothing(label, triangular):
    name = "several_tiles_s1000_triangular" if triangular else "several_tiles_s1000_rectangular"
    assert PAIR_CASES[name]["count_a"][[5, 11, 17]].tolist() == [1000, 1000, 1000]
    for pairs_device in (False, True):
        got = lib_pairs(PAIR_CASES[name], pairs_device=pairs_device, changes=BAD_SIGNATURES[label])
        assert got[0] == FA_ERR_INVALID and got[2] == -1 and untouched(got), (got[0], got[2], got[3], _lib.last_error())
    check_pairs(name, lib_pairs(PAIR_CASES[name]))                          # the process goes on


def test_bad_parameters_return_nothing():
    case = PAIR_CASES["named_s64_triangular"]
    for replaced in (dict(s=0), dict(s=4097), dict(jn=-1), dict(jn=2, jd=1), dict(jd=0)):
        got = lib_pairs(case, **replaced)
        assert got[0] == FA_ERR_INVALID and got[2] == -1 and untouched(got), replaced


def test_the_same_input_gives_the_same_bytes():
    name = "tile_s64_65_triangular"
    runs = [lib_pairs(PAIR_CASES[name], pairs_device=True) for _ in range(3)]
    for run in runs:
        check_pairs(name, run)
        assert run[1].tobytes() == runs[0][1].tobytes()


# ---- groups ----------------------------------------------------------------------------------------------------------
def lib_groups(records, n, pairs_device, labels_device):
    labels = np.full(n * 4, 0xAB, dtype=np.uint8)
    n_groups = C.c_int32(-1)
    d_records = to_device(records.view(np.int32)) if pairs_device else None
    d_labels = torch.from_numpy(labels.copy()).to(DEVICE) if labels_device else None
    torch.cuda.synchronize()
    code = lib.fa_screen_groups(ptr(d_records) if pairs_device else C.c_void_p(records.ctypes.data), len(records), int(pairs_device), n,
                                C.c_void_p(d_labels.data_ptr()) if labels_device else C.c_void_p(labels.ctypes.data), int(labels_device),
                                C.byref(n_groups))
    return code, (d_labels.cpu().numpy() if labels_device else labels), n_groups.value


@pytest.mark.parametrize("name", sorted(sc.group_cases()))
def test_groups_match_the_labels_written_by_hand(name):
    records, n, labels, n_groups = sc.group_cases()[name]
    for pairs_device in (False, True):
        for labels_device in (False, True):
            code, got, got_groups = lib_groups(records, n, pairs_device, labels_device)
            assert code == FA_OK, _lib.last_error()
            assert got.view(np.int32).tolist() == labels and got_groups == n_groups


def test_groups_of_screened_pairs_match_the_union_find():
    name = "tile_s64_65_triangular"
    records = expected_pairs(name)[0]
    want, want_groups = sc.restate_groups(records, 65)
    code, got, got_groups = lib_groups(records, 65, True, True)
    assert code == FA_OK and got.tobytes() == want.tobytes() and got_groups == want_groups and 1 < want_groups < 65


@pytest.mark.parametrize("edge", [(3, 3), (4, 2), (-1, 2), (2, 10)])
def test_a_bad_edge_is_invalid_and_leaves_the_labels_untouched(edge):
    records = sc.edge_records([(0, 1), edge, (2, 3)])
    for pairs_device in (False, True):
        code, labels, n_groups = lib_groups(records, 10, pairs_device, True)
        assert code == FA_ERR_INVALID and np.all(labels == 0xAB) and n_groups == -1, _lib.last_error()


# ---- the Python face, end to end ---------------------------------------------------------------------------------------
def as_signatures(case_set, k=16):
    sig, count = case_set
    return screen.Signatures(to_device(sig).view(len(count), -1), to_device(count), [f"g{i}" for i in range(len(count))], k)


def test_python_pairs_cut_by_distance():
    case = PAIR_CASES["several_tiles_s1000_triangular"]
    sigs = as_signatures((case["sig_a"], case["count_a"]))
    everything, _ = sc.restate_pairs(dict(case, jn=0, jd=1))
    for cut in (0.07, 0.12, 1.0):
        want = everything[screen.distance(everything, 16) <= cut]
        stats = {}
        got = screen.pairs(sigs, max_distance=cut, stats=stats)
        assert got.dtype == SCREEN_DTYPE and got.tobytes() == want.tobytes() and 0 < len(want)
        assert stats["evaluated"] == 19 * 18 // 2 and len(want) <= stats["kept"] <= len(everything)
        on_device = screen.pairs(sigs, max_distance=cut, device=True)
        assert on_device.is_cuda and on_device.dtype == torch.int32 and screen.to_records(on_device).tobytes() == want.tobytes()
    assert len(screen.pairs(sigs, max_distance=0.07)) < len(screen.pairs(sigs, max_distance=0.12)) < len(everything)
    rect = screen.pairs(sigs, sigs, max_distance=0.12)
    tri = screen.pairs(sigs, max_distance=0.12)
    assert rect[rect["a"] < rect["b"]].tobytes() == tri.tobytes() and np.sum(rect["a"] == rect["b"]) == np.sum(case["count_a"] > 0)
    first, rest = as_signatures((case["sig_a"][:4], case["count_a"][:4])), as_signatures((case["sig_a"][4:], case["count_a"][4:]))
    joined = screen.Signatures.concat([first, rest])
    assert len(joined) == 19 and joined.names[4] == "g0" and screen.pairs(joined, max_distance=0.12).tobytes() == tri.tobytes()
    with pytest.raises(ValueError, match="do not compare"):
        screen.pairs(sigs, as_signatures((case["sig_a"], case["count_a"]), k=21))
    labels = screen.groups(tri, 19)
    assert isinstance(labels, np.ndarray) and labels.tobytes() == sc.restate_groups(tri, 19)[0].tobytes()
    on_device = screen.groups(screen.pairs(sigs, max_distance=0.12, device=True), 19)
    assert on_device.is_cuda and on_device.cpu().numpy().tobytes() == labels.tobytes()
    near = screen.groups(tri, 19, max_distance=0.07, k=16)
    assert near.tobytes() == sc.restate_groups(tri[screen.distance(tri, 16) <= 0.07], 19)[0].tobytes()


def test_families_end_to_end(tmp_path):
    """Twelve genomes in three families: the signatures of a real sketch are those of the restatement on the records read back,
    the groups are the families, and the sketch indexes and answers afterwards as one that was never screened."""
    import pyfastani_amd as pf
    genomes = sc.family_genomes()
    sketch, untouched_sketch = pf.Sketch(), pf.Sketch()
    for i, genome in enumerate(genomes):
        sketch.add_genome(f"genome{i}", genome)
        untouched_sketch.add_genome(f"genome{i}", genome)
    sigs = screen.signatures(sketch, size=1000)
    assert len(sigs) == 12 and sigs.size == 1000 and sigs.k == sketch.k == 16 and sigs.names == sketch.names
    rec, (lengths, sbf, counter) = sketch._export_records("cuda")
    rec = rec.cpu().numpy()
    want_sig, want_count = sc.restate_signatures({"hash": rec[0].view(np.uint32), "seq_id": rec[1], "sbf": np.asarray(sbf, dtype=np.int32), "s": 1000})
    assert sigs.count.cpu().numpy().tobytes() == want_count.tobytes() and np.all(want_count == 1000)
    assert sigs.sig.cpu().numpy().tobytes() == want_sig.tobytes()
    small = screen.signatures(sketch, size=64)
    assert small.sig.cpu().numpy().tobytes() == np.ascontiguousarray(want_sig[:, :64]).tobytes()
    records = screen.pairs(sigs, max_distance=0.2)
    want, _ = sc.restate_pairs(sc.pair_case((want_sig, want_count), (want_sig, want_count), 1000, True))
    assert records.tobytes() == want[screen.distance(want, 16) <= 0.2].tobytes()
    assert all(r["a"] // 4 == r["b"] // 4 for r in records) and len(records) >= 9
    labels = screen.groups(records, 12)
    assert labels.tolist() == [0] * 4 + [4] * 4 + [8] * 4
    assert screen.partition(labels) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]
    outputs.write_screen(tmp_path / "screen.tsv", sigs.names, sigs.names, records, sigs.k)
    lines = (tmp_path / "screen.tsv").read_text().splitlines()
    assert len(lines) == len(records) and lines[0].startswith("genome0\tgenome1\t0.0") and lines[0].endswith("/1000")
    # the screened sketch is whole: same records, same index, same answer
    mapper, plain = sketch.index(), untouched_sketch.index()
    for query in (genomes[5], genomes[0][:40_000]):
        got = [(h.name, h.identity, h.matches, h.fragments) for h in mapper.query_genome(query)]
        assert got == [(h.name, h.identity, h.matches, h.fragments) for h in plain.query_genome(query)] and len(got) >= 3
