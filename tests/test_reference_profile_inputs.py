"""The inputs of the reference-profile tests are what their names claim, the restatement (reference_profile.py) agrees with a
second definition written with dicts and `fractions.Fraction`, and the end-to-end family does through the CPU oracle what the
GPU test relies on -- no GPU."""
import ctypes as C
from fractions import Fraction

import numpy as np

import fragment_profile as fp
import reference_profile as rp
from pyfastani_amd import _lib


def chunks():
    R, E = C.c_int32(0), C.c_int32(0)
    assert _lib.lib.fa_reference_profile_chunk(C.byref(R)) == _lib.FA_OK and _lib.lib.fa_profile_regions_chunk(C.byref(E)) == _lib.FA_OK
    return R.value, E.value


def define(case, maps):
    """the profile by its definition: {bin: [count, sum in fixed-point units rounded per record, lowest]}"""
    first_bin = [int(x) for x in case["contig_bin"]]
    entries, stats = {}, [0, 0, 0]
    for m in maps:
        q, r, c, p, x = int(m["query_id"]), int(m["ref_genome_id"]), int(m["ref_seq_id"]), int(m["ref_start_pos"]), np.float32(m["identity"])
        assert 0 <= q < case["n_queries"] and 0 <= r < case["n_references"] and 0 <= c < len(first_bin) - 1
        assert int(case["contig_genome"][c]) == r and 0 <= p and p // case["bin_length"] < first_bin[c + 1] - first_bin[c]
        if not x >= np.float32(case.get("min_identity", 0.0)):
            stats[2] += 1
            continue
        if case.get("query_labels") is not None and int(case["query_labels"][q]) != int(case["reference_labels"][r]):
            stats[1] += 1
            continue
        if case.get("self_reference") is not None and int(case["self_reference"][q]) == r:
            stats[1] += 1
            continue
        stats[0] += 1
        exact = Fraction(float(x)) * 2 ** 20
        below = exact.numerator // exact.denominator
        rest = exact - below
        unit = below + (1 if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and below % 2 == 1) else 0)      # half to even, spelled out
        e = entries.setdefault(first_bin[c] + p // case["bin_length"], [0, 0, np.float32(np.inf)])
        e[0], e[1], e[2] = e[0] + 1, e[1] + unit, min(e[2], x)
    return entries, stats


def define_regions(count, total, offsets, need, below, min_length):
    """the regions by their definition: the maximal sets of consecutive holding entries of one segment, found from the set of
    holding entries rather than by a walk that carries a run"""
    out = []
    for s in range(len(offsets) - 1):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        holding = {i for i in range(lo, hi) if (int(count[i]) < int(need[s])) == bool(below)}
        for first in sorted(i for i in holding if i == lo or i - 1 not in holding):
            end = first
            while end in holding:
                end += 1
            if end - first >= min_length:
                out.append((s, first - lo, end - first, 0, sum(int(count[i]) for i in range(first, end)),
                            sum(int(total[i]) for i in range(first, end)) if total is not None else 0))
    return out


def test_the_chunk_constants():
    R, E = chunks()
    assert R >= 256 and R % 256 == 0 and E >= 256 and E % 256 == 0
    assert 2 * R + 1 <= int(rp.LAYOUT["contig_bin"][-1])          # a query can hold 2R + 1 records on distinct bins
    assert _lib.lib.fa_reference_profile_chunk(None) == _lib.FA_ERR_INVALID and _lib.lib.fa_profile_regions_chunk(None) == _lib.FA_ERR_INVALID


def test_restatement_against_the_definition():
    g = np.random.default_rng(32)
    layout = {"bin_length": 7, "contig_bin": np.array([0, 3, 3, 4, 9], dtype=np.int32), "contig_genome": np.array([0, 1, 1, 2], dtype=np.int32),
              "n_references": 3}
    for trial in range(12):
        n = int(g.integers(0, 200))
        ident = np.where(g.random(n) < 0.3, g.integers(0, 4, n) / 2.0 ** 21 * 3 + 90, 80 + 20 * g.random(n)).astype(np.float32)
        maps = rp.records_on_bins(layout, g.integers(0, 4, n), g.integers(0, 9, n), ident, g)
        case = dict(layout, n_queries=4, maps=maps)
        if trial % 2:
            case.update(query_labels=g.integers(0, 2, 4), reference_labels=g.integers(0, 2, 3))
        if trial % 3 == 0:
            case["self_reference"] = g.integers(-1, 3, 4)
        if trial % 4 == 0 and n:
            case["min_identity"] = float(ident[0])
        count, total, lowest, stats = rp.restate(case)
        entries, want_stats = define(case, maps)
        assert stats == want_stats and sum(stats) == n
        for i in range(len(count)):
            c, s, low = entries.get(i, [0, 0, np.float32(np.inf)])
            assert (int(count[i]), int(total[i])) == (c, s) and lowest[i].tobytes() == np.float32(low).tobytes()
        cut = n // 3
        again = rp.restate(case, maps[cut:], into=rp.restate(case, maps[:cut])[:3])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], (count, total, lowest)))


def test_regions_restatement_against_the_definition():
    g = np.random.default_rng(33)
    for trial in range(40):
        lengths = g.integers(0, 9, int(g.integers(0, 6)))
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        count = g.integers(0, 4, int(offsets[-1])).astype(np.int32)
        total = g.integers(0, 1000, len(count)).astype(np.int64) if trial % 3 else None
        need = g.integers(0, 4, len(lengths)).astype(np.int32)
        for below in (False, True):
            for min_length in (1, 2, 3):
                got = rp.regions(count, total, offsets, need, below, min_length)
                assert got.dtype == rp.REGION and got.tolist() == define_regions(count, total, offsets, need, below, min_length)


def test_cases_are_what_their_names_claim():
    R, _ = chunks()
    cases = rp.cases(R)
    cb, cg = rp.LAYOUT["contig_bin"], rp.LAYOUT["contig_genome"]
    assert len(cg) == 5 and len(set(cg.tolist())) == 3 and np.diff(cb).tolist().count(0) == 1 and np.diff(cb).tolist().count(1) == 1
    for name, case in cases.items():
        assert rp.refusal(case, case["maps"]) is None, name
    assert [len(cases[f"one_query_{n}"]["maps"]) for n in (0, 1, R - 1, R, R + 1, 2 * R + 1)] == [0, 1, R - 1, R, R + 1, 2 * R + 1]
    # the mapper's order: (query, reference genome, bin), at most one record per (query, bin)
    for name in [f"one_query_{n}" for n in (R - 1, R, R + 1, 2 * R + 1)] + ["sorted"]:
        m = cases[name]["maps"]
        bins = cb[m["ref_seq_id"]].astype(np.int64) + m["ref_start_pos"] // rp.BIN_LENGTH
        assert np.array_equal(np.lexsort((bins, m["ref_genome_id"], m["query_id"])), np.arange(len(m))), name
        assert len(set(zip(m["query_id"].tolist(), bins.tolist()))) == len(m), name
        assert int(rp.restate(cases[name])[0].max()) <= cases[name]["n_queries"]
    one = cases["one_bin"]
    assert len(one["maps"]) == 2 * R + 1 == one["n_queries"] == len(set(one["maps"]["query_id"].tolist()))
    count = rp.restate(one)[0]
    assert int(count.max()) == 2 * R + 1 and int((count > 0).sum()) == 1
    s, sh = cases["sorted"]["maps"], cases["shuffled"]["maps"]
    assert len(s) > R and sorted(x.tobytes() for x in s) == sorted(x.tobytes() for x in sh) and s.tobytes() != sh.tobytes()
    # the last bin of every contig that has bins, at the bin's first and last base
    last = cases["last_bins"]["maps"]
    assert set(last["ref_seq_id"].tolist()) == {0, 2, 3, 4}
    bins = last["ref_start_pos"] // rp.BIN_LENGTH
    assert (bins == (cb[1:] - cb[:-1])[last["ref_seq_id"]] - 1).all()
    assert set((last["ref_start_pos"] % rp.BIN_LENGTH).tolist()) == {0, rp.BIN_LENGTH - 1}
    # every filter drops something and keeps something, alone and together
    for name in ("labels", "self", "labels_and_self"):
        stats = rp.restate(cases[name])[3]
        assert stats[0] > 0 and stats[1] > 0 and stats[2] == 0, (name, stats)
    assert rp.restate(cases["labels_and_self"])[3][1] > max(rp.restate(cases[n])[3][1] for n in ("labels", "self"))
    eq, ab = cases["min_identity_equal"], cases["min_identity_above"]
    hit = int((s["identity"] == np.float32(eq["min_identity"])).sum())
    assert hit >= 1 and np.float32(ab["min_identity"]) == np.nextafter(np.float32(eq["min_identity"]), np.float32(np.inf))
    assert rp.restate(eq)[3][2] + hit == rp.restate(ab)[3][2] and rp.restate(eq)[3][2] > 0
    both = rp.restate(cases["min_identity_and_filters"])[3]
    assert both[0] > 0 and both[1] > 0 and both[2] > 0
    ends = cases["half_units_and_ends"]["maps"]["identity"]
    halves, _ = fp.half_unit_identities()
    assert set(halves.tolist()) <= set(ends.tolist()) and 0.0 in ends and 128.0 in ends and not np.signbit(ends).any()


def test_refused_calls_have_one_fault_each():
    R, _ = chunks()
    got = rp.refused(R)
    assert set(got) == set(rp.REFUSED_FOR)
    for name, (case, bad) in got.items():
        assert rp.refusal(case, bad) == rp.REFUSED_FOR[name], name
        good = dict(case, bin_length=rp.BIN_LENGTH, contig_bin=rp.LAYOUT["contig_bin"])
        assert rp.refusal(good, good["maps"]) is None
        differ = [i for i in range(len(bad)) if bad[i].tobytes() != good["maps"][i].tobytes()]
        assert differ == ([] if name in ("bin_length_zero", "contig_bin_decreases") else [R + 5]), name
    # the position faults: exactly the contig's bins times the bin length, and a bin that exists -- in the next contig
    case, bad = got["position_at_the_end"]
    assert int(bad["ref_start_pos"][R + 5]) == 40 * rp.BIN_LENGTH and int(bad["ref_seq_id"][R + 5]) == 0 and int(case["contig_bin"][1]) == 40
    case, bad = got["position_in_the_next_contig_s_bins"]
    assert int(case["contig_bin"][0]) + int(bad["ref_start_pos"][R + 5]) // rp.BIN_LENGTH == 40 < int(case["contig_bin"][-1])
    case, bad = got["contig_of_another_genome"]
    assert int(case["contig_genome"][int(bad["ref_seq_id"][R + 5])]) != int(bad["ref_genome_id"][R + 5])
    assert int(bad["ref_start_pos"][R + 5]) // rp.BIN_LENGTH < 25


def test_region_case_is_what_it_claims():
    _, E = chunks()
    case = rp.region_case(E)
    assert case["lengths"][:6] == [0, 1, E - 1, E, E + 1, 3 * E + 5]
    off = case["offsets"]
    got = rp.regions(case["count"], case["sum"], off, case["need"])
    assert not (got["segment"] == 0).any() and got[got["segment"] == 1].tolist()[0][1:3] == (0, 1)
    runs = {(int(r["segment"]), int(r["first"])): int(r["length"]) for r in got}
    assert runs[(3, 0)] == 3 and any(s == 3 and f + n == E for (s, f), n in runs.items())          # first entry; last entry
    # one run crosses the chunk boundary at 4E, one spans the chunks 4, 5 and 6; both lie in segment 5
    first = 4 * E - 3 - int(off[5])
    assert runs[(5, first)] == 7 and int(off[5]) < 4 * E - 3
    first = 4 * E + 10 - int(off[5])
    assert runs[(5, first)] == 2 * E - 7 and 6 * E + 3 < int(off[6])
    # the two segments of 7 hold everywhere and give two regions
    assert runs[(6, 0)] == 7 and runs[(7, 0)] == 7 and int(off[7]) - int(off[6]) == 7
    longest = int(got["length"].max())
    assert longest == 2 * E - 7 and len(rp.regions(case["count"], case["sum"], off, case["need"], min_length=longest + 1)) == 0
    assert 0 < len(rp.regions(case["count"], case["sum"], off, case["need"], min_length=2)) < len(got)
    # need 0: everything holds, one region per segment that has entries; below 0 nothing does
    zero = np.zeros(len(case["lengths"]), np.int32)
    everything = rp.regions(case["count"], case["sum"], off, zero)
    assert everything["length"].tolist() == [n for n in case["lengths"] if n] and not len(rp.regions(case["count"], case["sum"], off, zero, below=True))
    assert int(everything["hits"].sum()) == int(case["count"].sum()) and int(everything["sum"].sum()) == int(case["sum"].sum())
    assert len(rp.regions(case["count"], case["sum"], off, case["need"], below=True)) > 0


def _oracle_family():
    from oracle.oracle import OracleSketch
    fam = fp.family()
    osk = OracleSketch()
    for i, contigs in enumerate(fam["genomes"]):
        osk.add_draft(i, contigs)                              # one contig each: refSeqId is the genome number
    osk.index()
    return fam, [osk.query_draft(fam["genomes"][q], threads=4, details=True)[1]["mappings"] for q in range(4)]


def test_family_through_the_oracle():
    """what the GPU test of the family rests on, from the oracle's L2 mappings: against genome 0 the members 1 to 3 start in
    every bin but those of the insert and the last; against any other member no two adjacent bins go without a start"""
    fam, mappings = _oracle_family()
    bin_length = fp.FRAGMENT - 20
    assert bin_length == 2980
    for q in (1, 2, 3):
        m = mappings[q]
        bins = set((m["rstart"][m["rseq"] == 0] // bin_length).tolist())
        assert bins == set(range(10)) | set(range(13, 23)), (q, sorted(bins))
    for q in range(4):
        m = mappings[q]
        for r in range(1, 4):
            if r == q:
                continue
            starts = set((m["rstart"][m["rseq"] == r] // bin_length).tolist())
            n_bins = (len(fam["genomes"][r][0]) - 1) // bin_length + 1
            inner = range(n_bins - 1)                           # (the contig's last bin never receives a start)
            missing = [b for b in inner if b not in starts]
            assert all(b + 1 not in missing for b in missing), (q, r, missing)
