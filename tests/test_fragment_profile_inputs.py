"""The inputs of the fragment-profile tests are what their names claim, and the restatement (fragment_profile.py) agrees with a
second definition written with dicts and `fractions.Fraction` -- no GPU."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import fragment_profile as fp
from pyfastani_amd import _lib


def chunk():
    R, L = C.c_int32(0), C.c_int32(0)
    assert _lib.lib.fa_profile_chunk(C.byref(R), C.byref(L)) == _lib.FA_OK
    return R.value, L.value


def define(case, maps):
    """the profile by its definition: {entry: [count, sum as a Fraction of fixed-point units rounded per record, lowest]}"""
    first = [0]
    for n in case["counts"]:
        first.append(first[-1] + int(n))
    entries, stats = {}, [0, 0, 0]
    for m in maps:
        q, f, r, x = int(m["query_id"]), int(m["query_seq_id"]), int(m["ref_genome_id"]), np.float32(m["identity"])
        assert 0 <= q < len(case["counts"]) and 0 <= f < case["counts"][q] and 0 <= r < case["n_references"]
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
        e = entries.setdefault(first[q] + f, [0, 0, np.float32(np.inf)])
        e[0], e[1], e[2] = e[0] + 1, e[1] + unit, min(e[2], x)
    return entries, stats


def test_the_chunk_constants_leave_two_workgroups_a_cu():
    R, L = chunk()
    assert R >= 256 and R % 256 == 0
    assert L >= 1666 and 2 * 16 * L <= 160 * 1024            # a 5 Mb genome fits; two workgroups' entries fit the LDS of a CU
    assert _lib.lib.fa_profile_chunk(None, None) == _lib.FA_ERR_INVALID


def test_restatement_against_the_definition():
    g = np.random.default_rng(31)
    for trial in range(12):
        counts = [int(x) for x in g.integers(0, 9, 4)]
        counts[int(g.integers(0, 4))] = 5                   # (at least one query has fragments)
        n_ref = int(g.integers(1, 6))
        live = [q for q in range(4) if counts[q]]
        n = int(g.integers(0, 200))
        q = g.choice(live, n)
        ident = np.where(g.random(n) < 0.3, g.integers(0, 4, n) / 2.0 ** 21 * 3 + 90, 80 + 20 * g.random(n)).astype(np.float32)
        maps = fp.records(q, g.integers(0, np.asarray(counts)[q]), g.integers(0, n_ref, n), ident, g)
        case = {"counts": counts, "n_references": n_ref, "maps": maps}
        if trial % 2:
            case.update(query_labels=g.integers(0, 2, 4), reference_labels=g.integers(0, 2, n_ref))
        if trial % 3 == 0:
            case["self_reference"] = g.integers(-1, n_ref, 4)
        if trial % 4 == 0 and n:
            case["min_identity"] = float(ident[0])
        count, total, lowest, stats = fp.restate(case)
        entries, want_stats = define(case, maps)
        assert stats == want_stats and sum(stats) == n
        for i in range(len(count)):
            c, s, low = entries.get(i, [0, 0, np.float32(np.inf)])
            assert (int(count[i]), int(total[i])) == (c, s) and lowest[i].tobytes() == np.float32(low).tobytes()
        # split over calls: the same
        cut = n // 3
        again = fp.restate(case, maps[cut:], into=fp.restate(case, maps[:cut])[:3])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], (count, total, lowest)))


def test_fixed_point_ties_go_to_even():
    halves, k = fp.half_unit_identities()
    assert halves.dtype == np.float32
    for x, base in zip(halves, k.tolist()):
        assert Fraction(float(x)) * 2 ** 20 == Fraction(2 * base + 1, 2)        # exactly half a unit
        assert fp.fixed(x) == (base if base % 2 == 0 else base + 1)
    assert {int(b) % 2 for b in k} == {0, 1}
    assert fp.fixed(np.float32(0.0)) == 0 and fp.fixed(np.float32(128.0)) == 128 << 20
    assert fp.fixed(np.float32(97.53)) == int(np.rint(np.float64(np.float32(97.53)) * 2.0 ** 20))


def test_cases_are_what_their_names_claim():
    R, L = chunk()
    cases = fp.cases(R, L)
    for name, case in cases.items():
        assert fp.refusal(case, case["maps"]) is None, name
    assert [len(cases[f"one_query_{n}"]["maps"]) for n in (0, 1, R - 1, R, R + 1, 2 * R + 1)] == [0, 1, R - 1, R, R + 1, 2 * R + 1]
    # the query changes exactly where the first chunk ends, one record before, one behind
    for name, first in (("boundary_exact", R), ("boundary_before", R - 1), ("boundary_behind", R + 1)):
        q = cases[name]["maps"]["query_id"]
        assert (q[:first] == 0).all() and (q[first:] == 1).all() and len(q) > first
        assert fp.on_chip_workgroups(cases[name], cases[name]["maps"], 2, R, L) == (2 if first == R else 1)
    three = cases["three_queries_in_a_chunk"]
    assert len(set(three["maps"]["query_id"][:R].tolist())) == 3 and three["counts"][1] == 0
    for n in (L - 1, L, L + 1):
        case = cases[f"fragments_{n}"]
        mine = case["maps"][case["maps"]["query_id"] == 1]
        assert case["counts"][1] == n and len(mine) == len(case["maps"]) <= R
        assert 0 in mine["query_seq_id"] and n - 1 in mine["query_seq_id"]
        assert fp.on_chip_workgroups(case, case["maps"], 2, R, L) == (1 if n <= L else 0)
        assert fp.on_chip_workgroups(case, case["maps"], 1, R, L) == 0
    one = cases["one_fragment"]
    assert len(one["maps"]) == 2 * R + 1 and len(set(one["maps"]["query_seq_id"].tolist())) == 1
    assert len(set(one["maps"]["ref_genome_id"].tolist())) == 2 * R + 1
    assert int(fp.restate(one)[0].max()) == 2 * R + 1
    # sorted as the mapper emits; shuffled: the same records in another order, every chunk mixed
    s, sh = cases["sorted"]["maps"], cases["shuffled"]["maps"]
    key = lambda m: (m["query_seq_id"], m["ref_genome_id"], m["query_id"])  # noqa: E731
    assert np.array_equal(np.lexsort(key(s)), np.arange(len(s)))
    assert sorted(x.tobytes() for x in s) == sorted(x.tobytes() for x in sh) and s.tobytes() != sh.tobytes()
    assert fp.on_chip_workgroups(cases["shuffled"], sh, 2, R, L) == 0 < fp.on_chip_workgroups(cases["sorted"], s, 2, R, L)
    # every filter drops something and keeps something, alone and together
    for name in ("labels", "self", "labels_and_self"):
        stats = fp.restate(cases[name])[3]
        assert stats[0] > 0 and stats[1] > 0 and stats[2] == 0, (name, stats)
    assert fp.restate(cases["labels_and_self"])[3][1] > max(fp.restate(cases[n])[3][1] for n in ("labels", "self"))
    # the cut-off is an identity of the records: equality counts, the next float above drops exactly those records
    eq, ab = cases["min_identity_equal"], cases["min_identity_above"]
    hit = int((s["identity"] == np.float32(eq["min_identity"])).sum())
    assert hit >= 1 and np.float32(ab["min_identity"]) == np.nextafter(np.float32(eq["min_identity"]), np.float32(np.inf))
    assert fp.restate(eq)[3][2] + hit == fp.restate(ab)[3][2] and fp.restate(eq)[3][2] > 0
    both = fp.restate(cases["min_identity_and_filters"])[3]
    assert both[0] > 0 and both[1] > 0 and both[2] > 0
    ends = cases["half_units_and_ends"]["maps"]["identity"]
    halves, _ = fp.half_unit_identities()
    assert set(halves.tolist()) <= set(ends.tolist()) and 0.0 in ends and 128.0 in ends
    assert not np.signbit(ends).any()


def test_refused_records_have_one_fault_each():
    R, _ = chunk()
    want = {"bad_query_high": "query", "bad_query_negative": "query", "fragment_equals_count": "fragment", "fragment_negative": "fragment",
            "bad_reference_high": "reference", "bad_reference_negative": "reference", "nan": "identity", "minus_zero": "identity",
            "above_128": "identity", "negative": "identity", "infinite": "identity"}
    got = fp.refused(R)
    assert set(got) == set(want)
    for name, (case, bad) in got.items():
        assert fp.refusal(case, case["maps"]) is None and fp.refusal(case, bad) == want[name], name
        differ = [i for i in range(len(bad)) if bad[i].tobytes() != case["maps"][i].tobytes()]
        assert differ == [R + 5], name                        # one record, in the second chunk
    case, bad = got["fragment_equals_count"]
    assert int(bad["query_seq_id"][R + 5]) == case["counts"][int(bad["query_id"][R + 5])]


def test_summary_inputs():
    trip = 256
    case = fp.summary_case(trip)
    assert 0 in case["counts"] and max(case["counts"]) > 3 * trip and trip in case["counts"] and trip + 1 in case["counts"]
    assert int(case["count"].min()) == 0 and int(case["count"].max()) == 6
    for n_sets in (1, 5):
        need = fp.summary_min_counts(len(case["counts"]), n_sets)
        assert need.shape == (n_sets, len(case["counts"])) and need.dtype == np.int32
    need = fp.summary_min_counts(len(case["counts"]), 5)
    assert (need[0] == 0).all() and (need[1] > case["count"].max()).all()
    fragments, hits, sums = fp.summarise(case["counts"], case["count"], case["sum"], need)
    assert fragments[0].tolist() == case["counts"] and not fragments[1].any() and not hits[1].any() and not sums[1].any()
    assert int(hits[0].sum()) == int(case["count"].sum()) and int(sums[0].sum()) == int(case["sum"].sum())
    assert (fragments[:, 1] == 0).all()                       # the genome without fragments


def test_family_insert_maps_to_no_other_member():
    """the oracle's L2 mappings of genome 0 against the family: the three fragments of the planted insert map to nothing but
    genome 0 itself, every other fragment of genome 0 maps to every other member"""
    from oracle.oracle import OracleSketch
    fam = fp.family()
    assert fam["fragments"] == [23, 20, 20, 20] and fam["insert_fragments"] == [10, 11, 12]
    assert fp.INSERT_AT % fp.FRAGMENT == 0 and fp.INSERT_LENGTH == 3 * fp.FRAGMENT
    osk = OracleSketch()
    for i, contigs in enumerate(fam["genomes"]):
        osk.add_draft(i, contigs)                              # one contig each: refSeqId is the genome number
    osk.index()
    _, det = osk.query_draft(fam["genomes"][0], threads=4, details=True)
    m = det["mappings"]
    others = m["rseq"] != 0
    assert not np.isin(m["qseq"][others], fam["insert_fragments"]).any()
    for member in (1, 2, 3):
        have = set(m["qseq"][m["rseq"] == member].tolist())
        assert have == set(range(23)) - set(fam["insert_fragments"]), (member, sorted(have))
