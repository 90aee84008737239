"""A mapper under each reading of the open rules (`pyfastani_amd.Rules`) against the oracle built with the matching FO_*
switches (rules_cases.py) -- MI355X only.

Every comparison is on every L2 mapping (fa_mapper_debug_mappings), every row (count and float32 identity bit for bit) and the hit
list; test_rules_inputs.py asserts that each case tells the reading it is run under from the default, so none of these can
pass because two readings happen to agree.  Cases that need an environment variable the library reads once per process
run in a fresh child process."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import rules_cases as rc
import pyfastani_amd as pf

pytestmark = pytest.mark.gpu


def records_equal(a, b, what):
    assert a.dtype == b.dtype and len(a) == len(b), (what, len(a), len(b))
    if a.tobytes() != b.tobytes():
        bad = [i for i in range(len(a)) if a[i].tobytes() != b[i].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(a)} records differ, first at {bad[0]}: device {a[bad[0]]} expected {b[bad[0]]}")


@pytest.mark.parametrize("case,reading", [(c, r) for c in rc.CASES for r in rc.GPU_READINGS[c]])
def test_a_mapper_follows_its_rules(case, reading):
    want = rc.expected(case, reading)
    for cell, want_cell in zip(rc.inputs(case), want):
        mapper = rc.new_mapper(cell, reading)
        assert mapper.rules == pf.Rules(**rc.READINGS[reading])
        rc.assert_same(rc.gpu_cell(mapper, cell), want_cell, f"case {case} {cell['params']} under {reading}")
    if case == "E":                                           # ... which is the default oracle's answer too
        base = rc.expected("E", "default")[0][0]
        assert all(want[0][0][what] == base[what] for what in ("l2", "rows", "hits"))


def test_one_mapper_under_one_reading_after_another():
    cell = rc.inputs("A")[0]
    mapper = rc.new_mapper(cell)
    assert mapper.rules == pf.Rules() and mapper.rules.is_default
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        batch = mapper.upload_genomes(cell["queries"])

        def step():
            rows, maps = batch.query_mappings()
            return rc.gpu_cell(mapper, cell), rows.tobytes(), maps.tobytes()

        first = step()
        rc.assert_same(first[0], rc.expected("A", "default")[0], "default, first")
        mapper.rules = pf.Rules(**rc.READINGS["all"])
        assert mapper.rules == pf.Rules(0.75, "fragment", "largest")
        second = step()
        rc.assert_same(second[0], rc.expected("A", "all")[0], "all three")
        assert second[1] != first[1]
        mapper.rules = pf.Rules(**rc.READINGS["all"])                 # (the rules it has: nothing happens)
        mapper.rules = pf.Rules()
        assert mapper.rules.is_default
        third = step()
        rc.assert_same(third[0], rc.expected("A", "default")[0], "default again")
        assert third[1] == first[1] and third[2] == first[2]          # byte for byte
        for a, b in zip(third[0], first[0]):
            assert a["l2"] == b["l2"] and a["rows"] == b["rows"] and a["hits"] == b["hits"] and a["kept"].tobytes() == b["kept"].tobytes()
    with pytest.raises(ValueError):
        mapper.rules = _bad_rules()
    assert mapper.rules.is_default
    with pytest.raises(TypeError):
        mapper.rules = "largest"


def _bad_rules():
    """An object that passes for a Rules with a value the library refuses (the C side validates on its own)."""
    r = pf.Rules()
    object.__setattr__(r, "l2_confidence", 1.0)
    return r


def test_every_entry_point_follows_the_mapper():
    cell = rc.inputs("B")[0]
    want = rc.expected("B", "all")[0]
    n = len(cell["queries"])
    mapper = rc.new_mapper(cell, "all")
    want_rows = [(q, g, c, np.float32(x).tobytes()) for q, per in enumerate(want) for g, c, x in per["rows"]]
    want_maps = np.concatenate([per["kept"] for per in want])

    def row_tuples(rows):
        return [(int(r["query_id"]), int(r["ref_genome_id"]), int(r["count_seq"]), np.float32(r["identity"]).tobytes()) for r in rows]

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # query_draft / query_draft_mappings, one query at a time
        for q, contigs in enumerate(cell["queries"]):
            assert rc.hit_tuples(mapper.query_draft(contigs)) == want[q]["hits"], q
            hits, maps = mapper.query_draft_mappings(contigs)
            assert rc.hit_tuples(hits) == want[q]["hits"], q
            kept = want[q]["kept"].copy()
            kept["query_id"] = 0
            parts = [kept[kept["ref_genome_id"] == name] for name, _, _, _ in want[q]["hits"]]
            records_equal(maps, np.concatenate(parts) if parts else kept[:0], f"query_draft_mappings, query {q}")
        # the resident batch
        batch = mapper.upload_genomes(cell["queries"])
        assert [rc.hit_tuples(h) for h in batch.query()] == [per["hits"] for per in want]
        assert row_tuples(batch.query_rows()) == want_rows
        rows, maps = batch.query_mappings()
        assert row_tuples(rows) == want_rows
        records_equal(maps, want_maps, "GenomeBatch.query_mappings")
        # ... and in windows of a small stage, range by range
        mapper.set_mapping_stage(37)
        got_rows, got_maps, genomes = [], [], 0
        for first, count, r, m in batch.iter_mappings():
            assert first == genomes
            genomes += count
            got_rows.append(r)
            got_maps.append(m)
        assert genomes == n
        assert row_tuples(np.concatenate(got_rows)) == want_rows
        records_equal(np.concatenate(got_maps), want_maps, "GenomeBatch.iter_mappings")


FORCED = {
    "events_retry": {"FA_EVENTS_CAP_MIN": "1000"},
    "events_split": {"FA_EVENTS_CAP_MAX": "60000", "FA_EVENTS_CAP_MIN": "1000"},
    "scan_order_0": {"FA_L2_SCAN_ORDER": "0"},
    "scan_order_1": {"FA_L2_SCAN_ORDER": "1"},
    "no_packed_geo": {"FA_NO_PACKED_GEO": "1"},
}


@pytest.mark.parametrize("name", sorted(FORCED))
def test_forced_paths_under_the_longer_slide(name, tmp_path):
    env = FORCED[name]
    out = tmp_path / f"{name}.npz"
    res = subprocess.run([sys.executable, rc.__file__, "A", "end", str(out)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout[-2000:] + res.stderr[-2000:]
    with np.load(out) as z:
        got = rc.unpack(z, rc.inputs("A"))
        repeats, parts = int(z["repeats"]), int(z["parts"])
    rc.assert_same(got[0], rc.expected("A", "end")[0], f"case A under end, {env}", in_parts=name == "events_split")
    if name == "events_retry":
        assert repeats > 0, repeats                      # the first part found no room for its events and ran again
    if name == "events_split":
        assert parts > 1, parts                          # the pass was cut into parts


def test_the_tie_key_of_fragment_zero():
    """cgi_ties="largest" with queries whose fragment 0 maps (case B's self-queries): with the plain number in the low word of the
    two atomicMax keys, locus 0 or fragment 0 could form key 0, which both tables read as empty."""
    cell = rc.inputs("B")[0]
    want = rc.expected("B", "ties")[0]
    mapper = rc.new_mapper(cell, "ties")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for q, contigs in enumerate(cell["queries"]):
            hits, maps = mapper.query_draft_mappings(contigs)
            mine = maps[maps["ref_genome_id"] == q]
            assert len(mine) and mine["query_seq_id"].min() == 0, q
            assert (0, q) in {(int(r["query_seq_id"]), int(r["ref_genome_id"])) for r in want[q]["kept"]}
            assert rc.hit_tuples(hits) == want[q]["hits"]


def test_default_rules_reproduce_the_committed_goldens():
    sys.path.insert(0, os.path.join(rc.ROOT, "tests", "golden"))
    from make_synthetic_goldens import build_case
    fixtures = json.load(open(os.path.join(rc.ROOT, "tests", "golden", "synthetic_goldens.json")))
    assert fixtures
    for fx in fixtures:
        case = fx["case"]
        refs, queries = build_case(case)
        for rules in (None, pf.Rules()):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sk = pf.Sketch(**case["params"], rules=rules)
                for i, r in enumerate(refs):
                    sk.add_draft(f"ref{i}", r)
                mapper = sk.index()
                for q, w in zip(queries, fx["queries"]):
                    assert [[h.name, h.identity, h.matches, h.fragments] for h in mapper.query_draft(q)] == w["hits"], case["name"]
                    assert len(rc.gpu_l2(mapper)) == w["n_mappings"]
