"""Index build, L1 and L2 on planted minimizer records -- MI355X only.

Every other GPU test of the mapper takes its reference records from sequences; here they are written record by record
(tests/planted.py, pinned without a GPU by tests/test_planted_inputs.py) and reach the library through `Sketch.__setstate__`, the
road of a pickled sketch and of the sharded index build: hashes next to the query's, at the ends of the rank structure's buckets
and of 32 bits; same-hash pairs on either side of the link rule; record distances around 2^13 and 2^16; clusters in the lookup
table; list lengths that steer the frequency walk through each branch; hit counts that meet the L1 minimum exactly or miss it by
one.  Each case is compared with the oracle on the same records at every stage, all by equality."""
import ctypes as C
import warnings

import numpy as np
import pytest

import planted as pl
import pyfastani_amd as pf
from pyfastani_amd._lib import check, lib
from test_gpu_parity import gpu_mappings, hit_tuples, links_match_their_definitions, oracle_mappings, quiet_sketch

pytestmark = pytest.mark.gpu

VARIANTS = pl.gpu_variants()


def l1_loci(mapper):
    cap = 1 << 16
    arr = [np.empty(cap, np.int32) for _ in range(4)]
    n = C.c_int64(0)
    check(lib.fa_mapper_debug_l1(mapper._h, *[a.ctypes.data for a in arr], cap, C.byref(n)))
    assert n.value <= cap
    got = {}
    for f, s, a, b in zip(*[a[: n.value].tolist() for a in arr]):
        got.setdefault(f, []).append((s, a, b))
    return got


def lookup(mapper, key):
    """(count, positions) of a hash in the lookup index; count -1 for a hash it does not hold (positions of short lists only)."""
    n = C.c_int64(0)
    check(lib.fa_mapper_lookup_count(mapper._h, key, C.byref(n)))
    if not 0 < n.value <= 8:
        return n.value, []
    seq, wpos = np.empty(max(n.value, 1), np.int32), np.empty(max(n.value, 1), np.int32)
    check(lib.fa_mapper_lookup_get(mapper._h, key, seq.ctypes.data, wpos.ctypes.data, n.value))
    return n.value, list(zip(seq[: n.value].tolist(), wpos[: n.value].tolist()))


@pytest.mark.parametrize("case", VARIANTS, ids=[c.id for c in VARIANTS])
def test_planted_case_matches_the_oracle_at_every_stage(case, monkeypatch):
    for key, val in case.env.items():
        monkeypatch.setenv(key, val)
    sk = quiet_sketch(pf.Sketch, **case.cell.params)
    sk.__setstate__(case.state())
    assert (sk.window_size, sk.k, sk.fragment_length) == (case.cell.w, case.cell.k, case.cell.frag)
    assert all(np.array_equal(x, y) for x, y in zip(sk.minimizers._arrays(), (case.h, case.s, case.w)))
    mapper = sk.index()
    osk = case.oracle()
    # the index: records, links, lookup table, frequency threshold
    assert all(np.array_equal(x, y) for x, y in zip(mapper.minimizers._arrays(), (case.h, case.s, case.w)))
    links_match_their_definitions(mapper)
    assert len(mapper.lookup_index) == osk.index_size
    assert mapper.occurences_threshold == osk.freq_threshold
    absent = next(x for x in range(1, 1 << 20) if osk.index_count(x) < 0)
    keys = case.keys + [absent, 0, pl.M32]
    for key in keys:
        count, positions = lookup(mapper, key)
        assert count == osk.index_count(key), hex(key)
        if 0 < count <= 8:
            at = np.flatnonzero(case.h == key)
            assert positions == list(zip(case.s[at].tolist(), case.w[at].tolist())), hex(key)
    # L1, L2 and the hits, twice on the same mapper and once through a resident batch
    ohits, det = osk.query_draft([case.query], details=True)
    assert len(oracle_mappings(det)) >= len(case.fragments)
    for attempt in range(2):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            hits = mapper.query_draft([case.query])
        got = l1_loci(mapper)
        for f, fr in enumerate(case.fragments):
            _, _, loci = osk.l1_fragment(fr.bytes)
            assert sorted(got.get(f, [])) == sorted(loci), (attempt, f)
        assert gpu_mappings(mapper) == oracle_mappings(det), attempt
        assert hit_tuples(hits) == ohits, attempt
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        batch = mapper.upload_genomes([[case.query]])
        assert [hit_tuples(h) for h in batch.query()] == [ohits]
    assert gpu_mappings(mapper) == oracle_mappings(det)
