"""The reference-side conservation profile and the regions of a profile on the device (fa_mappings_reference_profile,
fa_profile_regions, fa_mapper_reference_bins, pyfastani_amd.conservation) against the plain restatement of reference_profile.py
-- MI355X only.  Every comparison is byte for byte."""
import ctypes as C

import numpy as np
import pytest
import torch

import fragment_profile as fp
import reference_profile as rp
from pyfastani_amd import _lib, conservation as cons
from pyfastani_amd._batch import MAPPING_DTYPE, REGION_DTYPE
from pyfastani_amd._lib import FA_ERR_INVALID, FA_OK, lib

pytestmark = pytest.mark.gpu


def chunks():
    R, E = C.c_int32(0), C.c_int32(0)
    assert lib.fa_reference_profile_chunk(C.byref(R)) == FA_OK and lib.fa_profile_regions_chunk(C.byref(E)) == FA_OK
    return R.value, E.value


R, E = chunks()
CASES = rp.cases(R)


def to_device(maps):
    return torch.from_numpy(np.ascontiguousarray(maps).view(np.int32).reshape(len(maps), 8).copy()).cuda()


def accumulators(start):
    return [torch.from_numpy(x.copy()).cuda() for x in start]


def host_i32(x):
    return np.ascontiguousarray(x, dtype=np.int32) if x is not None else None


def ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def add(case, maps, acc, device_records=True):
    """one fa_mappings_reference_profile call into the device accumulators `acc`: (code, stats)"""
    cb, cg = host_i32(case["contig_bin"]), host_i32(case["contig_genome"])
    ql, rl, sr = (host_i32(case.get(k)) for k in ("query_labels", "reference_labels", "self_reference"))
    stats = (C.c_int64 * 3)(-7, -7, -7)
    if device_records:
        records = to_device(maps)
        where = C.c_void_p(records.data_ptr())
    else:
        records = np.ascontiguousarray(maps, dtype=MAPPING_DTYPE)
        where = C.c_void_p(records.ctypes.data)
    torch.cuda.synchronize()
    code = lib.fa_mappings_reference_profile(where, len(maps), 1 if device_records else 0, case["n_queries"], case["n_references"], len(cg),
                                             ptr(cb), ptr(cg), case["bin_length"], ptr(ql), ptr(rl), ptr(sr),
                                             float(case.get("min_identity", 0.0)), *[C.c_void_p(a.data_ptr()) for a in acc], stats)
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
        _WANT[id(case)] = (case, rp.restate(case))            # (the case is kept: its id stays its own)
    return _WANT[id(case)][1]


def run_case(name, case, pieces=None, device_records=True):
    pieces = [case["maps"]] if pieces is None else pieces
    acc = accumulators(rp.empty(case))
    total = [0, 0, 0]
    for piece in pieces:
        code, stats = add(case, piece, acc, device_records)
        assert code == FA_OK, (name, _lib.last_error())
        total = [a + b for a, b in zip(total, stats)]
    count, sums, lowest, want_stats = wanted(case)
    same(acc, (count, sums, lowest), name)
    assert total == want_stats and sum(total) == len(case["maps"]), (name, total, want_stats)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_against_the_restatement(name):
    run_case(name, CASES[name])


@pytest.mark.parametrize("parts", [2, 5])
def test_split_over_calls(parts):
    case = CASES["labels_and_self"]
    cuts = np.linspace(0, len(case["maps"]), parts + 1).astype(int)
    run_case(f"split_{parts}", case, [case["maps"][a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    run_case("with_an_empty_call", case, [case["maps"][:100], case["maps"][:0], case["maps"][100:]])


def test_host_records():
    for name in ("sorted", "min_identity_and_filters", "half_units_and_ends", "last_bins"):
        run_case(name, CASES[name], device_records=False)


def test_accumulating_onto_a_profile_that_is_not_empty():
    case = CASES["sorted"]
    first = wanted(CASES["shuffled"])[:3]
    acc = accumulators(first)
    code, _ = add(case, case["maps"], acc)
    assert code == FA_OK
    same(acc, rp.restate(case, into=first)[:3], "twice")


@pytest.mark.parametrize("name", sorted(rp.refused(R)))
def test_refused_calls_leave_the_accumulators(name):
    case, bad = rp.refused(R)[name]
    good = dict(case, bin_length=rp.BIN_LENGTH, contig_bin=rp.LAYOUT["contig_bin"])
    before = wanted(CASES["sorted"])[:3]                          # (a profile of the same layout that already holds something)
    assert rp.refusal(good, good["maps"]) is None
    for device_records in (True, False):
        acc = accumulators(before)
        code, stats = add(case, bad, acc, device_records)
        assert code == FA_ERR_INVALID and _lib.last_error(), name
        assert stats == [-7] * 3
        same(acc, before, name)


# ---- the summary and the Python layer --------------------------------------------------------------------------------
def filled_profile(case):
    profile = cons.ReferenceProfile((case["bin_length"], case["contig_bin"], case["contig_genome"]), case["n_queries"])
    count, sums, lowest, _ = wanted(case)
    profile.count.copy_(torch.from_numpy(count))
    profile.sum.copy_(torch.from_numpy(sums))
    profile.lowest.copy_(torch.from_numpy(lowest))
    return profile


def test_summary_per_reference_genome():
    case = CASES["sorted"]
    profile = filled_profile(case)
    assert profile.n_references == 3 and profile.genome_bin.tolist() == [0, 40, 17041, 17066]
    count, sums = wanted(case)[:2]
    need = np.array([[0, 0, 0], [1, 2, 1], [2, 1, 3], [5, 5, 5]], dtype=np.int32)
    sizes = np.diff(profile.genome_bin)
    want = fp.summarise(sizes, count, sums, need)
    got = profile.summary(need)
    for have, expect in zip(got, want):
        assert have.cpu().numpy().tobytes() == expect.tobytes()
    assert want[0][0].tolist() == sizes.tolist() and int(want[1][0].sum()) == int(count.sum())
    share = profile.covered_fraction(need[1]).cpu().numpy()
    assert np.array_equal(share, want[0][1] / sizes)
    mean = profile.mean().cpu().numpy()
    assert np.array_equal(np.isnan(mean), count == 0) and np.array_equal(mean[count > 0], sums[count > 0] / count[count > 0] / 2.0 ** 20)


def test_python_layer_add():
    case = CASES["min_identity_and_filters"]
    profile = cons.ReferenceProfile((case["bin_length"], case["contig_bin"], case["contig_genome"]), case["n_queries"])
    stats = {}
    cut = len(case["maps"]) // 2
    kwargs = dict(query_labels=case["query_labels"], reference_labels=case["reference_labels"], self_reference=case["self_reference"],
                  min_identity=case["min_identity"], stats=stats)
    profile.add(case["maps"][:cut], **kwargs)                    # host records
    profile.add(to_device(case["maps"][cut:]), **kwargs)         # device records
    count, sums, lowest, want = wanted(case)
    same((profile.count, profile.sum, profile.lowest), (count, sums, lowest), "python")
    assert [stats[k] for k in ("counted", "skipped", "below")] == want
    bad = case["maps"][:5].copy()
    bad["ref_start_pos"][2] = -1
    with pytest.raises(ValueError, match="position"):
        profile.add(bad)
    same((profile.count, profile.sum, profile.lowest), (count, sums, lowest), "after a refusal")


# ---- the regions -----------------------------------------------------------------------------------------------------
def regions_call(case, need=None, below=0, min_length=1, with_sum=True, out_device=False, cap=None, count_only=False):
    """(code, records written or None, *n_regions, the untouched rest of the buffer)"""
    count, sums = torch.from_numpy(case["count"]).cuda(), torch.from_numpy(case["sum"]).cuda()
    need = np.ascontiguousarray(case["need"] if need is None else need, dtype=np.int32)
    want = rp.regions(case["count"], case["sum"] if with_sum else None, case["offsets"], need, below, min_length)
    cap = len(want) + 3 if cap is None else cap
    if out_device:
        out = torch.full((max(cap, 1), 8), -7, dtype=torch.int32, device="cuda")
        where = C.c_void_p(out.data_ptr())
    else:
        out = np.full((max(cap, 1), 8), -7, dtype=np.int32)
        where = ptr(out)
    n = C.c_int64(-7)
    torch.cuda.synchronize()
    code = lib.fa_profile_regions(C.c_void_p(count.data_ptr()), C.c_void_p(sums.data_ptr()) if with_sum else None, len(case["lengths"]),
                                  ptr(case["offsets"]), ptr(need), below, min_length,
                                  None if count_only else where, cap, C.byref(n), 1 if out_device else 0)
    got = np.ascontiguousarray(out.cpu().numpy() if out_device else out).view(REGION_DTYPE).reshape(-1)
    return code, got, n.value, want


def check_regions(case, **kwargs):
    code, got, n, want = regions_call(case, **kwargs)
    assert code == FA_OK, _lib.last_error()
    assert n == len(want) and got[:n].tobytes() == want.tobytes(), (kwargs, n, len(want))
    assert (got[n:].view(np.int32) == -7).all()                   # nothing behind the records is written
    return want


@pytest.mark.parametrize("out_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("below", [0, 1])
def test_regions_against_the_restatement(below, out_device):
    case = rp.region_case(E)
    want = check_regions(case, below=below, out_device=out_device)
    assert len(want) > 4
    if not below:
        # the two adjacent segments that hold everywhere are two regions
        assert want[-2:].tolist() == [(6, 0, 7, 0, 21, int(case["sum"][-14:-7].sum())), (7, 0, 7, 0, 21, int(case["sum"][-7:].sum()))]


def test_regions_min_length_and_need_zero():
    case = rp.region_case(E)
    longest = int(rp.regions(case["count"], case["sum"], case["offsets"], case["need"])["length"].max())
    assert len(check_regions(case, min_length=1)) > len(check_regions(case, min_length=2)) > 0
    assert len(check_regions(case, min_length=longest)) == 1 and len(check_regions(case, min_length=longest + 1)) == 0
    zero = np.zeros(len(case["lengths"]), np.int32)
    assert check_regions(case, need=zero)["length"].tolist() == [n for n in case["lengths"] if n]
    assert len(check_regions(case, need=zero, below=1)) == 0
    assert len(check_regions(case, below=1, min_length=2)) > 0


def test_regions_without_sum_and_counting_only():
    case = rp.region_case(E)
    want = check_regions(case, with_sum=False)
    assert not want["sum"].any() and want["hits"].any()
    code, got, n, want = regions_call(case, count_only=True)
    assert code == FA_OK and n == len(want) and (got.view(np.int32) == -7).all()


@pytest.mark.parametrize("out_device", [False, True], ids=["host", "device"])
def test_regions_into_a_buffer_one_short(out_device):
    case = rp.region_case(E)
    want = rp.regions(case["count"], case["sum"], case["offsets"], case["need"])
    code, got, n, _ = regions_call(case, cap=len(want) - 1, out_device=out_device)
    assert code == FA_ERR_INVALID and b"smaller" in lib.fa_last_error()
    assert n == len(want) and (got.view(np.int32) == -7).all()
    check_regions(case, cap=len(want), out_device=out_device)     # exactly enough


def test_regions_of_small_profiles():
    # no segment; one empty segment; one entry that holds and one that does not
    for lengths, count in (([], []), ([0], []), ([0, 0], []), ([1], [3]), ([1], [0]), ([2, 0, 1], [3, 3, 3])):
        case = {"lengths": lengths, "offsets": np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64),
                "count": np.array(count + [9], dtype=np.int32)[:len(count)], "sum": np.arange(len(count), dtype=np.int64) + 5,
                "need": np.full(len(lengths), 2, np.int32)}
        check_regions(case)
        check_regions(case, below=1)


def test_regions_through_the_python_layer():
    case = rp.region_case(E)
    # the reference side: the segments as contigs of three genomes, need per genome
    contig_genome = np.array([0, 0, 0, 1, 1, 1, 2, 2], dtype=np.int32)
    profile = cons.ReferenceProfile((2980, case["offsets"].astype(np.int32), contig_genome), 4)
    profile.count.copy_(torch.from_numpy(case["count"]))
    profile.sum.copy_(torch.from_numpy(case["sum"]))
    for need, below, min_length in ((2, False, 1), ([1, 2, 3], False, 2), ([3, 1, 2], True, 1)):
        per_contig = np.full(8, need, np.int32) if isinstance(need, int) else np.asarray(need, np.int32)[contig_genome]
        got = profile.regions(need, below=below, min_length=min_length)
        want = rp.regions(case["count"], case["sum"], case["offsets"], per_contig, below, min_length)
        assert got.dtype == REGION_DTYPE and got.tobytes() == want.tobytes() and len(want) > 0
    # the query side: two genomes of several contigs, one contig too short to hold a fragment
    lengths = [[7000, 2500, 9100], [3000, 12000]]
    fragments = cons.FragmentProfile([5, 5], 3)
    count = np.array([3, 3, 0, 3, 3, 3, 3, 1, 3, 3], dtype=np.int32)
    sums = (count.astype(np.int64) << 26) + np.arange(10)
    fragments.count.copy_(torch.from_numpy(count))
    fragments.sum.copy_(torch.from_numpy(sums))
    offsets = np.array([0, 2, 2, 5, 6, 10], dtype=np.int64)
    for need, below, min_length in (([2, 2], False, 1), ([2, 4], True, 1), (2, False, 2)):
        per_contig = np.repeat(np.full(2, need, np.int32) if isinstance(need, int) else np.asarray(need, np.int32), [3, 2])
        got = fragments.regions(lengths, 3000, need, below=below, min_length=min_length)
        want = rp.regions(count, sums, offsets, per_contig, below, min_length)
        assert got.tobytes() == want.tobytes() and len(want) > 0
    # fragments 0 and 1 end their contig, fragment 3 starts the next one with entries: two regions, not one
    first = fragments.regions(lengths, 3000, 2)
    assert first[["segment", "first", "length"]].tolist()[:3] == [(0, 0, 2), (2, 1, 2), (3, 0, 1)]


# ---- the bin numbering of a mapper -----------------------------------------------------------------------------------
def test_reference_bins_of_a_small_index():
    import pyfastani_amd as pf
    from pyfastani_amd import synthetic as syn
    g = syn.rng(99)
    # genome 0: contigs of 10 000 and 7 000; genome 1: 5 (no minimizer window fits: no record, no bin), 4 000 and 30 000; genome 2: 9 000
    genomes = [[10_000, 7_000], [5, 4_000, 30_000], [9_000]]
    sk = pf.Sketch()
    for i, lengths in enumerate(genomes):
        sk.add_draft(i, [syn.to_ascii(syn.random_codes(g, n)) for n in lengths])
    mapper = sk.index()
    bin_length, contig_bin, contig_genome = mapper.reference_bins()
    assert bin_length == 2980 and contig_bin.dtype == np.int32 and contig_genome.dtype == np.int32
    assert contig_genome.tolist() == [0, 0, 1, 1, 1, 2] and len(contig_bin) == 7 and contig_bin[0] == 0
    _, seq, wpos = mapper._read_minimizers()
    want = [int(wpos[seq == c].max()) // bin_length + 1 if (seq == c).any() else 0 for c in range(6)]
    assert np.diff(contig_bin).tolist() == want and want[2] == 0 and want[4] >= 10
    # the sizes alone
    n, b = C.c_int64(-1), C.c_int32(-1)
    assert lib.fa_mapper_reference_bins(C.c_void_p(mapper._h), C.byref(b), C.byref(n), None, None) == FA_OK and (b.value, n.value) == (2980, 6)
    profile = cons.ReferenceProfile(mapper, 1)
    assert profile.n_references == 3 and profile.genome_bin.tolist() == [0, int(contig_bin[2]), int(contig_bin[5]), int(contig_bin[6])]
    assert profile.count.device == mapper._torch_device() and len(profile.count) == int(contig_bin[-1])


# ---- end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def family_results():
    mapper, batch = fp.family_mapper()
    counts = [int(x) for x in batch.total_fragments]
    fragments = cons.FragmentProfile(counts, 4, device=mapper._torch_device())
    stats = {}
    profile, rows = cons.reference_all_vs_all(mapper, batch, self_reference=np.arange(4), stats=stats, fragment_profile=fragments)
    plain, plain_rows = cons.all_vs_all(mapper, batch, self_reference=np.arange(4))
    plain_rows2, maps = batch.query_mappings()
    return {"profile": profile, "fragments": fragments, "rows": rows, "plain": plain, "plain_rows": plain_rows, "maps": maps,
            "stats": stats, "bins": mapper.reference_bins()}


def test_family_reference_profile_equals_the_restatement_of_the_library_s_records(family_results):
    r = family_results
    bin_length, contig_bin, contig_genome = r["bins"]
    assert bin_length == fp.FRAGMENT - 20 and contig_genome.tolist() == [0, 1, 2, 3]
    case = {"bin_length": bin_length, "contig_bin": contig_bin, "contig_genome": contig_genome, "n_references": 4, "n_queries": 4,
            "maps": r["maps"], "self_reference": np.arange(4)}
    count, sums, lowest, stats = rp.restate(case)
    same((r["profile"].count, r["profile"].sum, r["profile"].lowest), (count, sums, lowest), "family")
    assert [r["stats"][k] for k in ("counted", "skipped", "below")] == stats and stats[0] > 0 and stats[1] > 0
    assert r["rows"].tobytes() == r["plain_rows"].tobytes()
    # the same device records fed the fragment profile: what conservation.all_vs_all gives
    same((r["fragments"].count, r["fragments"].sum, r["fragments"].lowest),
         [x.cpu().numpy() for x in (r["plain"].count, r["plain"].sum, r["plain"].lowest)], "fragment profile")


def test_family_insert_is_an_island_of_the_reference(family_results):
    r = family_results
    profile = r["profile"]
    count = profile.count.cpu().numpy()
    assert int(profile.genome_bin[0]) == 0 and (count[10:13] == 0).all()      # (genome 0: its bins start at 0)
    islands = profile.regions(3, below=True, min_length=2)
    assert islands[["segment", "first", "length"]].tolist() == [(0, 10, 3)] and int(islands["hits"][0]) == 0
    rows = r["rows"]
    pairs = rows[rows["query_id"] != rows["ref_genome_id"]]
    assert len(pairs) == 12 and int(count.sum()) == int(pairs["count_seq"].sum())
    # per reference genome: every other member's records land in it
    for g in range(4):
        mine = pairs[pairs["ref_genome_id"] == g]
        assert int(count[profile.genome_bin[g]:profile.genome_bin[g + 1]].sum()) == int(mine["count_seq"].sum())


def test_ranges_of_a_table_give_the_bytes_of_one_call():
    mapper, batch = fp.family_mapper()
    one = cons.ReferenceProfile(mapper, 4)
    pieces = cons.ReferenceProfile(mapper, 4)
    _, maps = batch.query_mappings()
    one.add(maps, self_reference=np.arange(4))
    n_ranges = 0
    for first, count in ((0, 1), (1, 2), (3, 1)):
        for _, _, _, device_maps in batch.iter_mappings_device(first=first, count=count):
            pieces.add(device_maps, self_reference=np.arange(4))
            n_ranges += 1
    assert n_ranges >= 3
    same((pieces.count, pieces.sum, pieces.lowest), [x.cpu().numpy() for x in (one.count, one.sum, one.lowest)], "ranges")
    assert int(one.count.sum()) > 0
