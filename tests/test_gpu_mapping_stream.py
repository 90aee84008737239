"""The fragment mappings as a stream (fa_mapper_query_genomes_mappings_stream / fa_mapper_query_mappings_stream, the binding's
query_mappings / iter_mappings on top of them) against the oracle's records (hit_mappings.expected) -- MI355X only.

The records leave the device in windows of S records (fa_mapper_set_mapping_stage).  Whatever S is, the records are the
expected ones byte for byte and in order, the rows are those of query_rows, and a sink sees, pass by pass, full windows and
one last ragged one.  The `passes` batch mapped as one pass is 14 x 276 bins: two chunks of the compaction, the second
ragged, about a thousand records -- at S = 1 a window edge falls behind every record, so between lanes of one 64-bin read,
between waves, between the chunks and on either side of the last record; the other sizes put a full window, the last record
and the end of the pass in every relation to one another.  Cases that need an environment variable before HIP starts run
mapping_stream.py as a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hit_mappings as hm
import mapping_stream as ms
from pyfastani_amd import _lib
from pyfastani_amd._batch import MAPPING_DTYPE

pytestmark = pytest.mark.gpu

REC = MAPPING_DTYPE.itemsize


def same(got, want, what):
    assert got.dtype == want.dtype and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ, first at {bad[0]}: device {got[bad[0]]} expected {want[bad[0]]}")


def windows(pass_records, S):
    """sizes of the sink calls: per pass full windows and a ragged last one, nothing for an empty pass"""
    out = []
    for n in pass_records:
        out += [S] * (n // S) + ([n % S] if n % S else [])
    return out


def run_child(case, env, stages, tmp_path, fresh=False):
    out = tmp_path / f"{case}.npz"
    res = subprocess.run([sys.executable, ms.__file__, case, str(out), ",".join(str(s) for s in stages)] + (["fresh"] if fresh else []),
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout[-2000:] + res.stderr[-2000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def one_pass_stages():
    n = sum(len(m) for m in hm.expected("passes")["maps"])
    divisors = [d for d in range(2, n) if n % d == 0]
    return n, sorted({1, 7, 64, n - 1, n, n + 1, 10 * n} | set(divisors[-1:]))


@pytest.fixture(scope="module")
def one_pass():
    return ms.sweep("passes", one_pass_stages()[1])


def test_stage_sweep_one_pass(one_pass):
    n, stages = one_pass_stages()
    want = np.concatenate(hm.expected("passes")["maps"])
    exp = hm.expected("passes")["maps"]
    assert len(exp[0]) and len(exp[13]) and len(stages) >= 7      # (records on both sides of the chunk boundary, in query 7's bins)
    got = one_pass
    for S in stages:
        k = f"s{S}_"
        same(got[k + "maps"], want, f"S={S} query_mappings")
        assert got[k + "rows"].tobytes() == got["plain_rows"].tobytes(), S
        assert int(got[k + "sink_code"]) == 0 and int(got[k + "sink_count"]) == n
        same(got[k + "sink_maps"], want, f"S={S} sink")
        assert got[k + "sink_rows"].tobytes() == got["plain_rows"].tobytes(), S
        sizes = got[k + "sink_sizes"].tolist()
        assert len(sizes) == -(-n // S) and sizes == windows([n], S), (S, sizes[:4], sizes[-2:])
        assert got[k + "iter_ranges"].tolist() == [[0, 14]]
        same(got[k + "iter_maps"], want, f"S={S} iter_mappings")
        assert got[k + "iter_rows"].tobytes() == got["plain_rows"].tobytes()
        assert int(got[k + "null_code"]) == 0 and int(got[k + "null_count"]) == n
        # one pass: the buffer entry without room reports the count of the call
        assert int(got[k + "old_code"]) == _lib.FA_ERR_INVALID and int(got[k + "old_count"]) == n


def test_stage_memory_is_fixed(one_pass):
    # the stage is 2 x S records in HBM and as many pinned, whatever the number of records ...
    assert one_pass["s64_memory"][:3].tolist() == [64, 2 * 64 * REC, 2 * 64 * REC] and int(one_pass["s64_memory"][3]) > 0
    assert one_pass["s1_memory"][:3].tolist() == [1, 2 * REC, 2 * REC]
    # ... also from a call that returns few records to one that returns more than ten times as many
    exp = hm.expected("passes")["maps"]
    small = min((q for q in range(len(exp)) if len(exp[q])), key=lambda q: len(exp[q]))
    mapper = ms.new_mapper("passes")
    batch = mapper.upload_genomes(hm.inputs("passes")["queries"])
    mapper.set_mapping_stage(64)
    _, few = batch.query_mappings(small, 1)
    before = mapper.mapping_memory()
    _, many = batch.query_mappings()
    after = mapper.mapping_memory()
    same(few, exp[small], "one genome")
    same(many, np.concatenate(exp), "all genomes")
    assert len(many) >= 10 * len(few) > 0
    assert before[:3] == after[:3] == (64, 2 * 64 * REC, 2 * 64 * REC)


def test_stage_sweep_seven_passes(tmp_path):
    exp = hm.expected("passes")["maps"]
    per_pass = [len(exp[q]) + len(exp[q + 1]) for q in range(0, 14, 2)]            # FA_PASS_FRAGMENTS=120: two genomes of 45 fragments
    n0, n = per_pass[0], sum(per_pass)
    first, count = hm.inputs("passes")["sub"]                                          # (3, 5): passes (3, 4), (5, 6), (7)
    sub_pass = [len(exp[3]) + len(exp[4]), len(exp[5]) + len(exp[6]), len(exp[7])]
    assert len(exp[5]) == 0 and n0 > 64 and min(per_pass) > 0
    stages = [7, 64, n0, n0 + 1]
    got = run_child("passes", {"FA_PASS_FRAGMENTS": "120"}, stages, tmp_path)
    want, want_sub = np.concatenate(exp), np.concatenate(exp[first:first + count])
    for S in stages:
        k = f"s{S}_"
        assert int(got[k + "parts"]) == 7
        same(got[k + "maps"], want, f"S={S} query_mappings")
        same(got[k + "sub_maps"], want_sub, f"S={S} sub-range")
        assert got[k + "rows"].tobytes() == got["plain_rows"].tobytes()
        keep = (got["plain_rows"]["query_id"] >= first) & (got["plain_rows"]["query_id"] < first + count)
        assert got[k + "sub_rows"].tobytes() == got["plain_rows"][keep].tobytes()
        # the sink: the windows of pass after pass; query 5, related to nothing, adds no record and no call
        same(got[k + "sink_maps"], want, f"S={S} sink")
        same(got[k + "sub_sink_maps"], want_sub, f"S={S} sub-range sink")
        assert got[k + "sink_sizes"].tolist() == windows(per_pass, S), (S, got[k + "sink_sizes"].tolist())
        assert got[k + "sub_sink_sizes"].tolist() == windows(sub_pass, S)
        assert 5 not in got[k + "sink_maps"]["query_id"]
        # iter_mappings: the seven passes, whose concatenation is query_mappings
        assert got[k + "iter_ranges"].tolist() == [[q, 2] for q in range(0, 14, 2)]
        same(got[k + "iter_maps"], want, f"S={S} iter_mappings")
        assert got[k + "iter_rows"].tobytes() == got["plain_rows"].tobytes()
        # the null sink counts the whole call; the buffer entry without room stops at the first pass
        assert int(got[k + "null_code"]) == 0 and int(got[k + "null_count"]) == n
        assert int(got[k + "old_code"]) == _lib.FA_ERR_INVALID and int(got[k + "old_count"]) == n0 < n


def test_void_parts_with_small_windows(tmp_path):
    # the mapping call is the mapper's first query and the speculated locus capacity is far too small: parts are void and run
    # again, the rows -- and with them the count, the scan and the first window -- are formed again
    got = run_child("one_part", {"FA_LOCI_CAP_MIN": "7"}, [7], tmp_path, fresh=True)
    want = np.concatenate(hm.expected("one_part")["maps"])
    assert int(got["s7_repeats"]) > 0, got["s7_repeats"]
    assert len(want) > 3 * 7
    same(got["s7_maps"], want, "first query of a fresh mapper")
    assert got["s7_rows"].tobytes() == got["plain_rows"].tobytes()
    same(got["s7_sink_maps"], want, "sink")
    assert got["s7_sink_sizes"].tolist() == windows([len(want)], 7)


@pytest.mark.parametrize("case,S", [("contested", 5), ("protein", 64)])
def test_one_query(case, S):
    import warnings
    hits, want = hm.expected_draft(case, 0)
    want_hits = np.array(hits, dtype=np.float64).reshape(-1, 4)
    if case == "protein":
        assert len(want) == 260                                                        # five windows of 64
    tup = lambda hs: np.array([(h.name, h.identity, h.matches, h.fragments) for h in hs], dtype=np.float64).reshape(-1, 4)  # noqa: E731
    mapper = ms.new_mapper(case)
    query = hm.inputs(case)["queries"][0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        before = tup(mapper.query_draft(query))
        mapper.set_mapping_stage(S)
        got_hits, got = mapper.query_draft_mappings(query)
        after = tup(mapper.query_draft(query))
    assert mapper.mapping_memory()[:3] == (S, 2 * S * REC, 2 * S * REC)
    assert np.array_equal(tup(got_hits), want_hits) and np.array_equal(before, want_hits) and np.array_equal(after, want_hits)
    same(got, want, "query_draft_mappings")


def test_sink_abort():
    exp = hm.expected("passes")["maps"]
    want = np.concatenate(exp)
    mapper = ms.new_mapper("passes")
    batch = mapper.upload_genomes(hm.inputs("passes")["queries"])
    plain = batch.query_rows()
    mapper.set_mapping_stage(7)
    sink = ms.Sink(stop_at=2)
    code, _, _ = ms.stream_call(mapper, batch, 0, len(batch), sink.ptr)
    assert code == _lib.FA_ERR_INVALID and "sink" in _lib.last_error(), (code, _lib.last_error())
    assert sink.sizes == [7, 7]                                                        # no call behind the one that said stop
    same(sink.records(), want[:7], "the window before the stop")
    # the workspace was handed back and the mapper works as before
    assert batch.query_rows().tobytes() == plain.tobytes()
    rows, maps = batch.query_mappings()
    same(maps, want, "after the abort")
    assert rows.tobytes() == plain.tobytes()
