"""The sketch, index and mapping kernels across the whole k-mer-size range -- MI355X only.

k picks the number of 16-byte blocks and the tail that hash_codes<0> / hash_bytes hash (k >> 4, k & 15; the tail's second
lane from a remainder of 9 on), the premixed forms (k = 14 / 16 / 21, whose neighbours take the generic form inside the same
k_sketch_fast), the k - 1 bases a tile stages behind its positions (more than the tile itself from k > 1024), and with
4^k k-mers at small k the tie rule of the window minimum, k_suppress_runs and the palindromes that leave positions without a
k-mer.  Lists, sequences and cells come from tests/kmer_domain.py; tests/test_kmer_domain_inputs.py holds them, the oracle's
hash and the cells' claims to what is stated here, without a GPU.  The minimizer streams are compared with the oracle at
every k of KS under every window of WS (one per form of K1) and, by the two properties of winnowing, with a hash written in
Python; the end-to-end cells compare mappings and hits with the oracle, mapping for mapping and bit for bit."""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import kmer_domain as kd
import test_gpu_window_domain as wd
from oracle.oracle import OracleSketch
from pyfastani_amd import _lib, diagnostics, synthetic as syn
from pyfastani_amd._lib import lib, check
from test_gpu_parity import gpu_mappings, hit_tuples, oracle_mappings
from test_gpu_window_domain import check_winnowing

pytestmark = pytest.mark.gpu


def params_for(k, w, alphabet=4):
    return _lib.Params(k, w, 3000, alphabet, 0.2, 80.0, 1e-3, 5_000_000)


def gpu_stream(p, seq):
    cap = max(len(seq), 1)
    h = np.empty(cap, np.uint32)
    wp = np.empty(cap, np.int32)
    n = C.c_int64(0)
    check(lib.fa_debug_sketch_sequence(C.byref(p), seq, len(seq), 1, h.ctypes.data, wp.ctypes.data, cap, C.byref(n)))
    assert n.value <= cap
    return h[: n.value], wp[: n.value]


# ----------------------------------------------------------------------------------------------------------------
# (a) streams against the oracle
# ----------------------------------------------------------------------------------------------------------------
def check_streams(k):
    g = syn.rng(9500 + k)
    for w in kd.WS:
        p, osk = params_for(k, w), kd.oracle_sketch(k, w)
        for name, seq in kd.stream_cases(k, w, g).items():
            gh, gw = gpu_stream(p, seq)
            oh, ow = osk.sketch_sequence(seq)
            assert np.array_equal(gh, oh) and np.array_equal(gw, ow), f"k={k} w={w} {name}: gpu {len(gh)} records, oracle {len(oh)}"
            assert len(oh) >= 1 or name not in kd.YIELDING, (k, w, name)


@pytest.mark.parametrize("k", kd.KS)
def test_kmer_domain_streams(k):
    check_streams(k)


@pytest.mark.parametrize("env", [{"FA_K1_GENERAL": "1"}, {"FA_K1_TILE": "1024"}], ids=["general", "full-tile"])
def test_kmer_domain_streams_through_the_other_forms(env):
    # every tile through the 64-bit window minimum / reference tiles of the full 1 024 positions: the same streams in a child
    # process (the knobs are read once per process), as tests/test_gpu_window_domain.py runs its own
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                          "-k", "test_kmer_domain_streams and not other_forms and not by_definition"],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and f"{len(kd.KS)} passed" in res.stdout, res.stdout[-3000:] + res.stderr[-2000:]


# ----------------------------------------------------------------------------------------------------------------
# (b) streams by definition, with a hash that owes nothing to the oracle
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", kd.DEFINITION_KS)
def test_kmer_domain_streams_by_definition(k, monkeypatch):
    g = syn.rng(9700 + k)
    for w in kd.DEFINITION_WS:
        p = params_for(k, w)
        for seq in kd.definition_cases(k, w, g):
            gh, gw = gpu_stream(p, seq)
            monkeypatch.setattr(wd, "murmur_hash", kd.HashOf(seq, k))      # what check_winnowing hashes with
            check_winnowing(seq, k, w, gh, gw)


# ----------------------------------------------------------------------------------------------------------------
# (c) protein streams
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", kd.PROTEIN_KS)
def test_kmer_domain_protein_streams(k):
    g = syn.rng(9800 + k)
    p, osk = params_for(k, 1, alphabet=20), OracleSketch(k=k, protein=True)
    assert osk.window_size == 1
    for name, seq in kd.protein_cases(k, g).items():
        gh, gw = gpu_stream(p, seq)
        oh, ow = osk.sketch_sequence(seq)
        assert np.array_equal(gh, oh) and np.array_equal(gw, ow), f"k={k} {name}: gpu {len(gh)} records, oracle {len(oh)}"
        assert len(oh) == max(0, len(seq) - k + 1)                          # w = 1, no strand: every k-mer is a record


# ----------------------------------------------------------------------------------------------------------------
# (d) end to end
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(kd.CELLS))
def test_kmer_domain_end_to_end(name):
    cell = kd.CELLS[name]
    k, w = cell["k"], cell["w"]
    assert k not in (14, 16, 21)                                             # no compiled (k, w) form, no fused stage below
    refs, queries = kd.build_cell(cell)
    sk, osk = kd.sketch_pair(k, w, cell["frag"], cell["minfrac"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, r in enumerate(refs):
            sk.add_draft(f"ref{i}", r)
            osk.add_draft(f"ref{i}", r)
        mapper = sk.index()
        osk.index()
        assert mapper.window_size == w and mapper.k == k
        want = []
        for q in queries:
            hits = mapper.query_draft(q)
            ohits, det = osk.query_draft(q, threads=8, details=True)
            assert gpu_mappings(mapper) == oracle_mappings(det)
            assert hit_tuples(hits) == ohits
            assert len(ohits) == cell["hits"] and (len(det["mappings"]["qseq"]) > 0) == cell["maps"], (name, ohits)
            ms = diagnostics.timings(mapper)
            assert ms.fused == 0 and (ms.unfused > 0 or not cell["maps"]), ms
            want.append(ohits)
        # the same genomes as one resident batch
        got = [hit_tuples(h) for h in mapper.upload_genomes(queries).query()]
    assert got == want
