"""The fragment mappings behind the hits (fa_mapper_query_mappings / fa_mapper_query_genomes_mappings) against the oracle's
L2 mapping list reduced by the restatement of computeCGI's steps 1-2 (hit_mappings.py) -- MI355X only.

Every case: the records equal the expected ones field for field (identities bit for bit) and in (query, reference genome,
bin) order; per pair their number is the row's count_seq and their float32 running sum over the count the row's identity.
Cases that need an environment variable run in a fresh child process (the library reads its hooks once)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hit_mappings as hm
import pyfastani_amd as pf
from pyfastani_amd import _batch, _lib
from pyfastani_amd._lib import lib

pytestmark = pytest.mark.gpu


def run_child(case, env, tmp_path, fresh=False):
    out = tmp_path / ("_".join([case] + [f"{k}{v}" for k, v in sorted(env.items())]) + ".npz")
    res = subprocess.run([sys.executable, hm.__file__, case, str(out)] + (["fresh"] if fresh else []), env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout[-2000:] + res.stderr[-2000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def test_one_query_one_part():
    # 3 pairs: the last workgroup of k_cgi_rows forms the rows and hands the pass over, so the records are complete only if
    # the emission ran in front of it.  check_against_expected also compares the batch road with the one-query road and
    # query_draft before and after with the oracle's hits
    got = hm.gpu_results("one_part")
    hm.check_against_expected("one_part", got)
    assert len(got["draft_hits"]) == 3 and np.array_equal(got["hits_before"], got["hits_after"])
    for hit, n in zip(got["draft_hits"], [int((got["draft_maps"]["ref_genome_id"] == h[0]).sum()) for h in got["draft_hits"]]):
        assert n == int(hit[2])


@pytest.mark.parametrize("env", [{}, {"FA_PASS_FRAGMENTS": "16"}, {"FA_EVENTS_CAP_MAX": "9000", "FA_PASS_FRAGMENTS": "50"}],
                         ids=["whole", "parts_of_16", "parts_of_50_and_event_cap"])
def test_bins_contested_across_parts(env, tmp_path):
    # fragments of different parts compete for the same reference bins and each side wins some
    # (test_hit_mappings_inputs.py): a bin's entry must follow its key from part to part
    got = run_child("contested", env, tmp_path, fresh=True)      # (the mapping call finds the cut itself: the mapper's first query)
    hm.check_against_expected("contested", got)
    # the calls really ran in parts: a part holds FA_PASS_FRAGMENTS fragments at most (the event capacity may cut further)
    frags = [sum(len(c) // 3000 for c in q) for q in hm.inputs("contested")["queries"]]
    if not env:
        assert int(got["draft_parts"]) == 1 and int(got["batch_parts"]) == 1
    else:
        per = int(env["FA_PASS_FRAGMENTS"])
        assert int(got["draft_parts"]) >= -(-frags[0] // per) > 1, (got["draft_parts"], frags)
        assert int(got["batch_parts"]) >= sum(-(-f // per) for f in frags), (got["batch_parts"], frags)   # (a pass takes whole genomes)


@pytest.mark.parametrize("env", [{"FA_LOCI_CAP_MIN": "7"}, {"FA_EVENTS_CAP_MIN": "1000"}, {"FA_LOCI_CAP_MIN": "3", "FA_EVENTS_CAP_MIN": "64"}],
                         ids=["loci", "events", "both"])
def test_void_parts_leave_no_trace(env, tmp_path):
    # speculated capacities below the real numbers: parts are void and run again.  A mapper learns its capacities in its first
    # query, so each road maps on a fresh mapper and the mapping call is its first query: the void parts and their repeats
    # run with the winner table on, which both calls must report
    got = run_child("one_part", env, tmp_path, fresh=True)
    assert int(got["draft_repeats"]) > 0 and int(got["batch_repeats"]) > 0, (got["draft_repeats"], got["batch_repeats"])
    hm.check_against_expected("one_part", got)


def test_several_passes_and_a_sub_range(tmp_path):
    # seven passes of two genomes; the sub-range starts inside a pass of the full range; query 5 has no record at all
    got = run_child("passes", {"FA_PASS_FRAGMENTS": "120"}, tmp_path)
    hm.check_against_expected("passes", got)
    assert int(got["batch_parts"]) == 7 and int(got["sub_parts"]) == 3      # passes (3, 4), (5, 6), (7) of the sub-range
    assert 5 not in got["maps"]["query_id"] and 5 not in got["maps"]["ref_genome_id"]
    assert sorted(set(got["maps"]["query_id"].tolist())) == [q for q in range(14) if q != 5]
    assert sorted(set(got["sub_maps"]["query_id"].tolist())) == [3, 4, 6, 7]


def test_capacity_is_checked():
    import torch
    inp = hm.inputs("one_part")
    want = np.concatenate(hm.expected("one_part")["maps"])
    n_true = len(want)
    sk = pf.Sketch()
    for i, contigs in enumerate(inp["refs"]):
        sk.add_draft(i, contigs)
    mapper = sk.index()
    batch = mapper.upload_genomes(inp["queries"])
    rows = (_lib.CgiRow * 8)()
    n_rows, n_maps = C.c_int64(0), C.c_int64(0)
    guard = 0x5A5A5A5A
    words = _batch.MAPPING_DTYPE.itemsize // 4
    # a device destination one record short, with guard words behind it: the kernel must not write there
    dev = torch.full(((n_true + 1) * words,), guard, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    code = lib.fa_mapper_query_genomes_mappings(mapper._h, batch._h, 0, 1, rows, 8, C.byref(n_rows), 0, dev.data_ptr(), n_true - 1,
                                                C.byref(n_maps), 1)
    assert code == _lib.FA_ERR_INVALID and "mapping buffer too small" in _lib.last_error()
    assert n_maps.value == n_true                                         # the full count is reported all the same
    tail = dev[(n_true - 1) * words:].cpu().numpy()
    assert (tail == guard).all(), tail
    # the same through a host destination
    host = np.full((n_true + 1) * words, guard, dtype=np.int32)
    code = lib.fa_mapper_query_genomes_mappings(mapper._h, batch._h, 0, 1, rows, 8, C.byref(n_rows), 0, host.ctypes.data, n_true - 1,
                                                C.byref(n_maps), 0)
    assert code == _lib.FA_ERR_INVALID and _lib.last_error() and (host[(n_true - 1) * words:] == guard).all()
    # enough room: both succeed and agree with the expected records
    code = lib.fa_mapper_query_genomes_mappings(mapper._h, batch._h, 0, 1, rows, 8, C.byref(n_rows), 0, host.ctypes.data, n_true,
                                                C.byref(n_maps), 0)
    assert code == 0 and n_maps.value == n_true and n_rows.value == 3
    assert host[: n_true * words].tobytes() == want.tobytes() and (host[n_true * words:] == guard).all()
    code = lib.fa_mapper_query_genomes_mappings(mapper._h, batch._h, 0, 1, rows, 8, C.byref(n_rows), 0, dev.data_ptr(), n_true,
                                                C.byref(n_maps), 1)
    assert code == 0 and n_maps.value == n_true
    got = dev.cpu().numpy()
    assert got[: n_true * words].tobytes() == want.tobytes() and (got[n_true * words:] == guard).all()


def test_protein_golden():
    got = hm.gpu_results("protein")
    hm.check_against_expected("protein", got)
    assert [(int(h[0]), int(h[2]), int(h[3])) for h in got["draft_hits"]] == [(0, 130, 176), (1, 130, 176)]
    assert [int((got["draft_maps"]["ref_genome_id"] == g).sum()) for g in (0, 1)] == [130, 130]
