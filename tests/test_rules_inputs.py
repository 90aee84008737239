"""The inputs of the rules tests distinguish the readings they are run under, the restated computeCGI follows the variant
oracle, the host arithmetic behind `Rules.l2_confidence` follows the oracle's, and the Python / C surface of the rules
(`pyfastani_amd.Rules`, ``Sketch(rules=...)``, fa_rules) behaves -- no GPU compute here."""
import ctypes as C
import pickle
import subprocess
import sys

import numpy as np
import pytest

import rules_cases as rc
import pyfastani_amd as pf
from pyfastani_amd import _lib
from pyfastani_amd._lib import lib, check

# What every (case, reading) of the GPU test must move against the DEFAULT oracle, of the quantities that test compares: the L2
# mappings (fa_mapper_debug_mappings), the rows, the hit lists, the records of the restated computeCGI.  The slide end moves
# mappings but no row at these sizes, the tie rule rows and records but no mapping; case A holds no equal-identity tie at all.
MUST_MOVE = {
    ("A", "ci"): {"l2", "rows", "hits"}, ("A", "end"): {"l2", "kept"}, ("A", "ties"): set(), ("A", "all"): {"l2", "rows", "hits"},
    ("B", "ci"): {"l2", "rows"}, ("B", "end"): {"l2"}, ("B", "ties"): {"rows", "hits", "kept"}, ("B", "all"): {"l2", "rows", "hits", "kept"},
    ("C", "ci"): {"l2", "rows", "hits"}, ("C", "end"): {"l2"}, ("C", "ties"): {"rows", "hits"}, ("C", "all"): {"l2", "rows", "hits"},
    ("D", "ci"): {"l2", "rows", "hits"}, ("D", "end"): {"l2"}, ("D", "ties"): {"rows", "hits"}, ("D", "all"): {"l2", "rows", "hits"},
}


def kept_moved(case, reading):
    a, b = rc.expected(case, "default"), rc.expected(case, reading)
    return [qa["kept"].tobytes() != qb["kept"].tobytes() for ca, cb in zip(a, b) for qa, qb in zip(ca, cb)]


@pytest.mark.parametrize("case,reading", sorted(MUST_MOVE))
def test_every_reading_moves_what_its_gpu_test_compares(case, reading):
    assert reading in rc.GPU_READINGS[case]
    m = rc.moved(case, reading)
    kept = kept_moved(case, reading)
    print(case, reading, m, "queries whose kept records move:", sum(kept))
    for what in MUST_MOVE[case, reading]:
        assert (sum(kept) if what == "kept" else m[what]) > 0, (case, reading, what, m)
    if reading in ("ci", "end", "all"):
        assert all(n > 0 for n in m["l2_per_cell"]), m          # every cell of case C on its own
    if reading == "end":
        assert m["rows"] == 0 and m["hits"] == 0                 # (why that comparison is on every L2 mapping)
    if reading == "ties":
        assert m["l2"] == 0                                      # (and why this one is on rows, hits and records)
    if (case, reading) == ("B", "ties"):
        # the hit list and the kept records of EVERY query move: fragment 0 of each self-query maps (the key-0 guard)
        assert m["hits"] == len(rc.inputs("B")[0]["queries"]) and all(kept)
        for q, per in enumerate(rc.expected("B", "ties")[0]):
            assert any(r["query_seq_id"] == 0 and r["ref_genome_id"] == q for r in per["kept"]), q
    if (case, reading) == ("C", "ties"):
        assert m["rows_per_cell"][:2] == [0, 0] and m["rows_per_cell"][2] > 0     # only the k = 21 cell holds ties


def test_every_rule_is_told_apart_somewhere():
    for reading, what in (("ci", "l2"), ("ci", "rows"), ("end", "l2"), ("ties", "rows"), ("ties", "kept")):
        assert any(what in MUST_MOVE[c, reading] for c in "ABCD"), (reading, what)


def test_the_slide_end_reaches_contig_ends_in_case_d():
    """The clamp of the longer slide to the contig's end is exercised: under slide_end="fragment" some mapping of case D moves on
    a contig whose end lies within a fragment length of it."""
    a, b = rc.expected("D", "default")[0][0], rc.expected("D", "end")[0][0]
    cell = rc.inputs("D")[0]
    ends, n = {}, 0
    for contigs in cell["refs"]:
        for c in contigs:
            ends[n] = len(c)
            n += 1
    only = set(b["l2"]) - set(a["l2"])
    assert only
    assert any(ends[rseq] - rstart < 2 * 3000 for _, rseq, rstart, _, _ in only), sorted(only)[:4]


@pytest.mark.parametrize("case", rc.CASES)
def test_restated_compute_cgi_follows_the_variant_oracle(case):
    for reading in rc.READINGS:
        for per_query in rc.expected(case, reading):
            for q in per_query:
                assert rc.rows_of(q["kept"]) == q["rows"], (case, reading)


def test_protein_golden_moves_under_no_reading():
    base = rc.expected("E", "default")[0][0]
    assert [(h[0], h[2], h[3]) for h in base["hits"]] == [(0, 130, 176), (1, 130, 176)]
    for reading in rc.READINGS:
        got = rc.expected("E", reading)[0][0]
        assert got["l2"] == base["l2"] and got["rows"] == base["rows"] and got["hits"] == base["hits"], reading


# ---- the host arithmetic ------------------------------------------------------------------------------------------------
oracle_threshold = rc.oracle_threshold


@pytest.mark.parametrize("ci", [0.75, 0.9])
def test_pass_threshold_matches_the_oracle(ci):
    olib = rc.oracle("default").lib()
    got = C.c_int(0)
    differ = 0
    for s in range(1, 301):
        check(lib.fa_pass_threshold(s, 16, 80.0, ci, C.byref(got)))
        assert got.value == oracle_threshold(olib, s, 16, 80.0, ci), (s, ci)
        assert got.value == pf.pass_threshold(s, 16, 80.0, ci)
        check(lib.fa_pass_threshold(s, 16, 80.0, 0.9, C.byref(got)))
        differ += got.value != pf.pass_threshold(s, confidence=0.75)
    assert differ > 100                                           # (the two intervals are different filters)


def test_pass_threshold_at_the_default_interval_is_todays_filter():
    ident, upper, got = C.c_float(0), C.c_float(0), C.c_int(0)
    for k, pid in ((16, 80.0), (14, 80.0), (21, 90.0), (16, 95.0)):
        for s in (1, 2, 17, 85, 150, 233, 300):
            want = s + 1
            for c in range(s + 1):
                check(lib.fa_mapping_identity(c, s, k, C.byref(ident), C.byref(upper)))
                if upper.value >= np.float32(pid):
                    want = c
                    break
            check(lib.fa_pass_threshold(s, k, pid, 0.9, C.byref(got)))
            assert got.value == want, (k, pid, s)


def test_pass_threshold_refuses_bad_arguments():
    got = C.c_int(0)
    for s, k, ci in ((0, 16, 0.9), (10, 0, 0.9), (10, 16, 0.0), (10, 16, 1.0), (10, 16, -0.5)):
        assert lib.fa_pass_threshold(s, k, 80.0, ci, C.byref(got)) == _lib.FA_ERR_INVALID
    assert lib.fa_pass_threshold(10, 16, 80.0, 0.9, None) == _lib.FA_ERR_INVALID


# ---- Rules ------------------------------------------------------------------------------------------------------------------
def test_rules_values():
    r = pf.Rules()
    assert (r.l2_confidence, r.slide_end, r.cgi_ties) == (0.9, "windows", "smallest") and r.is_default
    assert repr(r) == "Rules(l2_confidence=0.9, slide_end='windows', cgi_ties='smallest')"
    a = pf.Rules(l2_confidence=0.75, slide_end="fragment", cgi_ties="largest")
    assert repr(a) == "Rules(l2_confidence=0.75, slide_end='fragment', cgi_ties='largest')" and not a.is_default
    assert eval(repr(a), {"Rules": pf.Rules}) == a
    assert a == pf.Rules(0.75, "fragment", "largest") and a != r and hash(a) == hash(pf.Rules(0.75, "fragment", "largest"))
    assert len({r, pf.Rules(), a, pf.Rules(cgi_ties="largest")}) == 3
    assert r != "Rules" and not (r == 0.9)
    b = pickle.loads(pickle.dumps(a))
    assert b == a and hash(b) == hash(a) and repr(b) == repr(a)
    with pytest.raises(AttributeError):
        a.slide_end = "windows"
    with pytest.raises(AttributeError):
        del a.cgi_ties
    with pytest.raises(AttributeError):
        a.extra = 1


@pytest.mark.parametrize("bad", [{"l2_confidence": 0.0}, {"l2_confidence": 1.0}, {"l2_confidence": -0.1}, {"l2_confidence": 1.5},
                                 {"l2_confidence": float("nan")}, {"l2_confidence": 1e-60}, {"slide_end": "window"}, {"slide_end": 1},
                                 {"slide_end": None}, {"cgi_ties": "biggest"}, {"cgi_ties": 0}])
def test_rules_refuse_other_values(bad):
    with pytest.raises(ValueError):
        pf.Rules(**bad)


def test_rules_need_a_number():
    with pytest.raises(TypeError):
        pf.Rules(l2_confidence="0.9")


def test_rules_import_without_numpy_or_torch():
    code = ("import sys; import pyfastani_amd as pf; r = pf.Rules(0.75, 'fragment', 'largest'); "
            "import pickle; assert pickle.loads(pickle.dumps(r)) == r; "
            "assert 'numpy' not in sys.modules and 'torch' not in sys.modules; print('OK')")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=rc.ROOT, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "OK", res.stdout + res.stderr


# ---- Sketch ---------------------------------------------------------------------------------------------------------------
def test_sketch_keeps_and_pickles_its_rules():
    rules = pf.Rules(0.75, "fragment", "largest")
    sk = pf.Sketch(rules=rules)
    assert sk.rules == rules and pf.Sketch().rules == pf.Rules() and pf.Sketch(rules=None).rules.is_default
    state = sk.__getstate__()
    assert state["rules"] == {"l2_confidence": 0.75, "slide_end": "fragment", "cgi_ties": "largest"}
    again = pickle.loads(pickle.dumps(sk))
    assert again.rules == rules and again.__getstate__() == state
    with pytest.raises(TypeError):
        pf.Sketch(None, None, None, None, None, None, None, rules)        # keyword-only, as every argument of the reference's signature
    with pytest.raises(TypeError):
        pf.Sketch(rules="largest")


def test_a_default_sketch_pickles_to_the_reference_state():
    state = pf.Sketch().__getstate__()
    assert sorted(state) == ["counter", "lengths", "names", "parameters", "sketch"]          # no "rules" key
    assert pf.Sketch(rules=pf.Rules()).__getstate__() == state
    other = pf.Sketch(rules=pf.Rules(cgi_ties="largest"))
    other.__setstate__(state)                                                              # a state without the key: the default
    assert other.rules.is_default
    other.__setstate__(dict(state, rules={"l2_confidence": 0.75, "slide_end": "windows", "cgi_ties": "smallest"}))
    assert other.rules == pf.Rules(l2_confidence=0.75)


def test_the_sharded_builders_forward_rules():
    """`build_index_sharded(**params)` and `build_ref_sharded_mapper(**params)` hand their keywords to `Sketch`."""
    import inspect
    from pyfastani_amd import sharding
    for fn in (sharding.build_index_sharded, sharding.build_ref_sharded_mapper):
        assert inspect.signature(fn).parameters["params"].kind is inspect.Parameter.VAR_KEYWORD
        assert "Sketch(**params)" in inspect.getsource(fn)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_struct_layout_and_default():
    assert C.sizeof(_lib.RulesStruct) == 12
    r = _lib.RulesStruct(0.0, 7, 7)
    check(lib.fa_rules_default(C.byref(r)))
    assert (r.l2_confidence, r.slide_end, r.cgi_ties) == (np.float32(0.9), 0, 0)
    assert lib.fa_rules_default(None) == _lib.FA_ERR_INVALID


def test_set_rules_reports_bad_arguments_without_a_device():
    good = _lib.RulesStruct(0.9, 0, 0)
    assert lib.fa_mapper_set_rules(None, C.byref(good)) == _lib.FA_ERR_INVALID and b"null mapper" in lib.fa_last_error()
    assert lib.fa_mapper_set_rules(None, None) == _lib.FA_ERR_INVALID
    assert lib.fa_mapper_get_rules(None, C.byref(good)) == _lib.FA_ERR_INVALID
    for bad, word in ((_lib.RulesStruct(0.0, 0, 0), b"l2_confidence"), (_lib.RulesStruct(1.0, 0, 0), b"l2_confidence"),
                      (_lib.RulesStruct(float("nan"), 0, 0), b"l2_confidence"), (_lib.RulesStruct(0.9, 2, 0), b"slide_end"),
                      (_lib.RulesStruct(0.9, -1, 0), b"slide_end"), (_lib.RulesStruct(0.9, 0, 2), b"cgi_ties")):
        assert lib.fa_mapper_set_rules(None, C.byref(bad)) == _lib.FA_ERR_INVALID
        assert word in lib.fa_last_error(), lib.fa_last_error()
