"""The per-fragment conservation profile on the device (fa_mappings_profile, fa_profile_summary,
pyfastani_amd.conservation) against the plain restatement of fragment_profile.py -- MI355X only.

Every case: count, sum, the bits of lowest and stats[0..2] equal the restatement byte for byte, under road 0 (the policy), 1
(global atomics) and 2 (on chip wherever it fits), and stats[3] shows that the intended road ran."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fragment_profile as fp
from pyfastani_amd import _lib, conservation as cons
from pyfastani_amd._batch import MAPPING_DTYPE
from pyfastani_amd._lib import FA_ERR_INVALID, FA_OK, lib

pytestmark = pytest.mark.gpu


def chunk():
    R, L = C.c_int32(0), C.c_int32(0)
    assert lib.fa_profile_chunk(C.byref(R), C.byref(L)) == FA_OK
    return R.value, L.value


R, L = chunk()
CASES = fp.cases(R, L)


@pytest.fixture(autouse=True)
def policy_road_afterwards():
    yield
    assert lib.fa_debug_profile_road(0) == FA_OK


def to_device(maps):
    return torch.from_numpy(np.ascontiguousarray(maps).view(np.int32).reshape(len(maps), 8).copy()).cuda()


def accumulators(start):
    return [torch.from_numpy(x.copy()).cuda() for x in start]


def host_i32(x):
    return np.ascontiguousarray(x, dtype=np.int32) if x is not None else None


def ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def add(case, maps, acc, device_records=True):
    """one fa_mappings_profile call into the device accumulators `acc`: (code, stats)"""
    off = fp.offsets_of(case["counts"])
    ql, rl, sr = (host_i32(case.get(k)) for k in ("query_labels", "reference_labels", "self_reference"))
    stats = (C.c_int64 * 4)(-7, -7, -7, -7)
    if device_records:
        records = to_device(maps)
        where = C.c_void_p(records.data_ptr())
    else:
        records = np.ascontiguousarray(maps, dtype=MAPPING_DTYPE)
        where = C.c_void_p(records.ctypes.data)
    torch.cuda.synchronize()
    code = lib.fa_mappings_profile(where, len(maps), 1 if device_records else 0, len(case["counts"]), ptr(off), case["n_references"],
                                   ptr(ql), ptr(rl), ptr(sr), float(case.get("min_identity", 0.0)),
                                   *[C.c_void_p(a.data_ptr()) for a in acc], stats)
    return code, list(stats)


def same(acc, want, what):
    for name, have, expect in zip(("count", "sum", "lowest"), acc, want):
        have = have.cpu().numpy()
        assert have.dtype == expect.dtype and have.tobytes() == expect.tobytes(), (what, name, np.nonzero(have.view(np.uint8).reshape(len(have), -1) !=
                                                                                                          expect.view(np.uint8).reshape(len(expect), -1))[0][:5])


_WANT = {}


def wanted(case):
    """the restatement of a case's own records, computed once"""
    if id(case) not in _WANT:
        _WANT[id(case)] = (case, fp.restate(case))            # (the case is kept: its id stays its own)
    return _WANT[id(case)][1]


def expected_on_chip(case, pieces, road):
    both = [sum(fp.on_chip_workgroups(case, p, r, R, L) for p in pieces if len(p)) for r in (1, 2)]
    return both if road == 0 else [both[road - 1]]


def run_case(name, case, road, pieces=None, device_records=True):
    assert lib.fa_debug_profile_road(road) == FA_OK
    pieces = [case["maps"]] if pieces is None else pieces
    acc = accumulators(fp.empty(case["counts"]))
    total = [0, 0, 0, 0]
    for piece in pieces:
        code, stats = add(case, piece, acc, device_records)
        assert code == FA_OK, (name, _lib.last_error())
        total = [a + b for a, b in zip(total, stats)]
    count, sums, lowest, want_stats = wanted(case)
    same(acc, (count, sums, lowest), (name, road))
    assert total[:3] == want_stats and sum(total[:3]) == len(case["maps"]), (name, road, total, want_stats)
    assert total[3] in expected_on_chip(case, pieces, road), (name, road, total[3])


@pytest.mark.parametrize("road", fp.ROADS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_against_the_restatement(name, road):
    run_case(name, CASES[name], road)


@pytest.mark.parametrize("road", fp.ROADS)
def test_the_roads_really_differ_in_what_ran(road):
    # one query of few fragments, 2R + 1 records: three workgroups, all on chip unless the road forbids it
    case = CASES[f"one_query_{2 * R + 1}"]
    assert lib.fa_debug_profile_road(road) == FA_OK
    acc = accumulators(fp.empty(case["counts"]))
    code, stats = add(case, case["maps"], acc)
    assert code == FA_OK and stats[3] in {0: (0, 3), 1: (0,), 2: (3,)}[road], stats
    # a query with more fragments than fit goes global on every road
    case = CASES[f"fragments_{L + 1}"]
    code, stats = add(case, case["maps"], accumulators(fp.empty(case["counts"])))
    assert code == FA_OK and stats[3] == 0


@pytest.mark.parametrize("road", fp.ROADS)
@pytest.mark.parametrize("parts", [2, 5])
def test_split_over_calls(parts, road):
    case = CASES["labels_and_self"]
    cuts = np.linspace(0, len(case["maps"]), parts + 1).astype(int)
    run_case(f"split_{parts}", case, road, [case["maps"][a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    # an empty call between two others touches nothing
    run_case("with_an_empty_call", case, road, [case["maps"][:100], case["maps"][:0], case["maps"][100:]])


@pytest.mark.parametrize("road", fp.ROADS)
def test_host_records(road):
    for name in ("sorted", "min_identity_and_filters", "half_units_and_ends"):
        run_case(name, CASES[name], road, device_records=False)


def test_accumulating_onto_a_profile_that_is_not_empty():
    case = CASES["sorted"]
    first = wanted(CASES["shuffled"])[:3]
    acc = accumulators(first)
    code, _ = add(case, case["maps"], acc)
    assert code == FA_OK
    same(acc, fp.restate(case, into=first)[:3], "twice")


@pytest.mark.parametrize("road", fp.ROADS)
@pytest.mark.parametrize("name", sorted(fp.refused(R)))
def test_refused_records_leave_the_accumulators(name, road):
    case, bad = fp.refused(R)[name]
    assert lib.fa_debug_profile_road(road) == FA_OK
    before = wanted(case)[:3]                                    # (a profile that already holds something)
    for device_records in (True, False):
        acc = accumulators(before)
        code, stats = add(case, bad, acc, device_records)
        assert code == FA_ERR_INVALID and _lib.last_error(), name
        assert stats == [-7] * 4
        same(acc, before, name)


def summary(case, need, out_device):
    off = fp.offsets_of(case["counts"])
    count, sums = torch.from_numpy(case["count"]).cuda(), torch.from_numpy(case["sum"]).cuda()
    n_sets, n = need.shape
    if out_device:
        out = [torch.full((n_sets, n), -7, dtype=torch.int64, device="cuda") for _ in range(3)]
        where = [C.c_void_p(x.data_ptr()) for x in out]
    else:
        out = [np.full((n_sets, n), -7, dtype=np.int64) for _ in range(3)]
        where = [ptr(x) for x in out]
    torch.cuda.synchronize()
    code = lib.fa_profile_summary(C.c_void_p(count.data_ptr()), C.c_void_p(sums.data_ptr()), n, ptr(off), ptr(need), n_sets, *where,
                                  1 if out_device else 0)
    assert code == FA_OK, _lib.last_error()
    return [x.cpu().numpy() if out_device else x for x in out]


@pytest.mark.parametrize("out_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n_sets", [1, 5])
def test_summary_against_the_restatement(n_sets, out_device):
    case = fp.summary_case(256)                                  # (256: one trip of a workgroup of the summary kernel)
    need = fp.summary_min_counts(len(case["counts"]), n_sets)
    got = summary(case, need, out_device)
    want = fp.summarise(case["counts"], case["count"], case["sum"], need)
    for name, have, expect in zip(("fragments", "hits", "sum"), got, want):
        assert have.tobytes() == expect.tobytes(), (name, have, expect)
    assert (got[0][:, 1] == 0).all()                             # the genome without fragments


def test_summary_of_many_sets_and_the_python_layer():
    case = fp.summary_case(256)
    g = np.random.default_rng(3)
    need = g.integers(0, 8, (11, len(case["counts"]))).astype(np.int32)          # three groups of sets, the last one short
    want = fp.summarise(case["counts"], case["count"], case["sum"], need)
    profile = cons.FragmentProfile(case["counts"], 9)
    profile.count.copy_(torch.from_numpy(case["count"]))
    profile.sum.copy_(torch.from_numpy(case["sum"]))
    got = profile.summary(need)
    for have, expect in zip(got, want):
        assert have.cpu().numpy().tobytes() == expect.tobytes()
    one = profile.summary(need[4])
    assert one.fragments.shape == (len(case["counts"]),) and one.hits.cpu().numpy().tobytes() == want[1][4].tobytes()
    share = profile.core_fraction(need[4]).cpu().numpy()
    counts = np.asarray(case["counts"])
    assert np.isnan(share[1]) and np.array_equal(np.delete(share, 1), np.delete(want[0][4] / np.maximum(counts, 1), 1))
    mean = profile.mean().cpu().numpy()
    assert np.array_equal(np.isnan(mean), case["count"] == 0)
    live = case["count"] > 0
    assert np.array_equal(mean[live], case["sum"][live] / case["count"][live] / 2.0 ** 20)
    with pytest.raises(ValueError):
        profile.summary(-need[4] - 1)


def test_python_layer_add():
    case = CASES["min_identity_and_filters"]
    profile = cons.FragmentProfile(case["counts"], case["n_references"])
    stats = {}
    cut = len(case["maps"]) // 2
    kwargs = dict(query_labels=case["query_labels"], reference_labels=case["reference_labels"], self_reference=case["self_reference"],
                  min_identity=case["min_identity"], stats=stats)
    profile.add(case["maps"][:cut], **kwargs)                    # host records
    profile.add(to_device(case["maps"][cut:]), **kwargs)         # device records
    count, sums, lowest, want = wanted(case)
    same((profile.count, profile.sum, profile.lowest), (count, sums, lowest), "python")
    assert [stats[k] for k in ("counted", "skipped", "below")] == want
    with pytest.raises(ValueError):
        profile.add(case["maps"], query_labels=case["query_labels"])
    bad = case["maps"][:5].copy()
    bad["query_seq_id"][2] = case["counts"][int(bad["query_id"][2])]
    with pytest.raises(ValueError, match="fragment"):
        profile.add(bad)
    same((profile.count, profile.sum, profile.lowest), (count, sums, lowest), "after a refusal")


# ---- end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def family_results():
    mapper, batch = fp.family_mapper()
    stats = {}
    profile, rows = cons.all_vs_all(mapper, batch, self_reference=np.arange(4), stats=stats)
    plain_rows, maps = batch.query_mappings()
    return {"profile": profile, "rows": rows, "plain_rows": plain_rows, "maps": maps, "stats": stats,
            "counts": [int(x) for x in batch.total_fragments]}


def test_family_profile_equals_the_restatement_of_the_library_s_records(family_results):
    r, fam = family_results, fp.family()
    assert r["counts"] == fam["fragments"] and r["rows"].tobytes() == r["plain_rows"].tobytes()
    case = {"counts": r["counts"], "n_references": 4, "maps": r["maps"], "self_reference": np.arange(4)}
    count, sums, lowest, stats = fp.restate(case)
    same((r["profile"].count, r["profile"].sum, r["profile"].lowest), (count, sums, lowest), "family")
    assert [r["stats"][k] for k in ("counted", "skipped", "below")] == stats and stats[0] > 0 and stats[1] > 0


def test_family_insert_is_novel_and_counts_add_up_to_the_rows(family_results):
    r, fam = family_results, fp.family()
    count = r["profile"].count.cpu().numpy()
    off = fp.offsets_of(r["counts"])
    assert (count[fam["insert_fragments"]] == 0).all()           # (genome 0: its entries start at 0)
    rest = np.delete(count[off[0]:off[1]], fam["insert_fragments"])
    assert rest.max() == 3                                        # shared with the three others (but for a bin lost to a neighbour)
    rows = r["rows"]
    for q in range(4):
        mine = rows[(rows["query_id"] == q) & (rows["ref_genome_id"] != q)]
        assert len(mine) == 3 and int(count[off[q]:off[q + 1]].sum()) == int(mine["count_seq"].sum())
    # the summary: the core of genome 0 at "all three others" and at "at least one other"
    need = np.array([[3, 3, 3, 3], [1, 1, 1, 1]], dtype=np.int32)
    got = r["profile"].summary(need)
    want = fp.summarise(r["counts"], count, r["profile"].sum.cpu().numpy(), need)
    for have, expect in zip(got, want):
        assert have.cpu().numpy().tobytes() == expect.tobytes()
    assert int(got.fragments[0, 0]) <= int(got.fragments[1, 0]) <= 20 and cons.min_count_for(np.zeros(4, np.int32), 1).tolist() == [3, 3, 3, 3]


def test_device_ranges_equal_query_mappings(tmp_path):
    # FA_PASS_FRAGMENTS = 25: every genome of the family (23, 20, 20, 20 fragments) is a range of its own
    out = tmp_path / "ranges.npz"
    res = subprocess.run([sys.executable, fp.__file__, str(out)], env=dict(os.environ, FA_PASS_FRAGMENTS="25"), capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout[-2000:] + res.stderr[-2000:]
    with np.load(out) as z:
        got = {k: z[k] for k in z.files}
    assert got["ranges"].tolist() == [[0, 1], [1, 1], [2, 1], [3, 1]]
    assert got["device_maps"].dtype == np.int32 and got["device_maps"].shape[1] == 8
    assert got["device_maps"].tobytes() == got["maps"].tobytes() and len(got["maps"]) > 0
    assert got["device_rows"].tobytes() == got["rows"].tobytes()


def test_a_short_device_buffer_raises():
    mapper, batch = fp.family_mapper()
    with pytest.raises(ValueError, match="mapping buffer too small"):
        for _ in batch.iter_mappings_device(max_records=10):
            pass
    with pytest.raises(ValueError):
        next(batch.iter_mappings_device(first=3, count=2))
