"""The inputs of the k-mer-size domain tests, checked without a GPU: the Python hash against the committed vectors, the
oracle's hash against the Python one at every critical k (the vectors stop at k = 100), and every end-to-end cell of
tests/test_gpu_kmer_domain.py against what it claims, with the oracle alone.  Lists, generators and cells come from
tests/kmer_domain.py, the module the GPU test takes them from."""
import json
import os

import numpy as np
import pytest

import kmer_domain as kd
from oracle.oracle import murmur_hash
from pyfastani_amd import synthetic as syn


def test_lists_are_the_stated_ones():
    assert kd.KS == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 15, 17, 20, 22, 24, 25, 31, 47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256,
                     257, 1000, 1023, 1024, 1025, 2047, 2048]
    assert kd.WS == [1, 2, 4, 24, 64, 65, 385, 1001]
    assert {k & 15 for k in kd.KS} >= {0, 1, 7, 8, 9, 15} and {k >> 4 for k in kd.KS} >= {0, 1, 2, 3, 128}
    assert kd.k1_tile_len(385) == 256 == kd.k1_tile_len(1001) and kd.k1_tile_len(24) == 976
    assert len(kd.CELLS) == len(kd.SMALL) + len(kd.MIDDLE) + len(kd.LARGE) + 2 * 6 * 2


def test_python_hash_equals_the_committed_vectors(golden_dir):
    vectors = json.load(open(os.path.join(golden_dir, "murmur3_vectors.json")))
    assert len(vectors) > 200
    for v in vectors:
        assert kd.murmur3_32(v["kmer"].encode("latin-1")) == v["hash"], v


@pytest.mark.parametrize("k", kd.KS)
def test_oracle_hash_equals_the_python_hash(k):
    """Seeded k-mers of every critical k, over ACGT and over arbitrary bytes: oracle.murmur_hash == murmur3_32 (which pins the
    oracle beyond the k = 100 of the vectors), and the array form of the Python hash equals the plain one."""
    g = syn.rng(9400 + k)
    seq = kd.rnd(g, k + 40)
    raw = bytes(g.integers(1, 256, k + 40, dtype=np.uint8))
    for s in (seq, raw):
        at_once = kd.murmur3_positions(s, k)
        assert len(at_once) == 41
        for i in range(41):
            want = kd.murmur3_32(s[i:i + k])
            assert murmur_hash(s[i:i + k]) == want == int(at_once[i]), (k, i)
    table = kd.HashOf(seq, k)
    assert table(seq[3:3 + k]) == kd.murmur3_32(seq[3:3 + k])
    rc = seq.translate(kd._RC)[::-1]
    assert table(rc[:k]) == kd.murmur3_32(rc[:k])


@pytest.mark.parametrize("k", [1, 2, 9, 48, 2048])
def test_stream_cases_hold_what_they_claim(k):
    """Every case meant to yield records holds three tiles, the halo and k bases, and yields records in the oracle; the AT
    repeat yields none at even k (every k-mer is its own reverse complement) and a sequence below k + w - 1 bases none."""
    for w in kd.WS:
        osk = kd.oracle_sketch(k, w)
        cases = kd.stream_cases(k, w, syn.rng(9500 + k))
        full = kd.full_length(k, w)
        for name in ("random", "two_letters", "ATGC_repeat", "ACGT_repeat", "polyA", "AT_repeat", "N_runs_longer_than_w",
                     "iupac_lower", "palindromes", "repeats"):
            assert len(cases[name]) >= full, (k, w, name)
        for name in kd.YIELDING:
            assert len(osk.sketch_sequence(cases[name])[0]) >= 1, (k, w, name)
        assert {len(cases[f"stretch_{n}"]) - (2 * (k + w) + 4) for n in ("k", "k_w_minus_2", "k_w_minus_1", "k_w")} == \
            {k, k + w - 2, k + w - 1, k + w}
        for name in ("shorter_than_k", "len_w_plus_k_minus_2"):
            assert len(osk.sketch_sequence(cases[name])[0]) == 0
        if k % 2 == 0:
            assert len(osk.sketch_sequence(cases["AT_repeat"])[0]) == 0
        assert any(c in cases["iupac_lower"] for c in b"RYKM") and cases["iupac_lower"][-1:].islower()


@pytest.mark.parametrize("name", list(kd.CELLS))
def test_cells_yield_what_they_claim(name):
    """The oracle alone: the listed number of hits (at least three where mappings are expected), a mapping list that is
    empty exactly where the cell says so, and no fragment with more than 8 192 seed hits inside one reference contig."""
    cell = kd.CELLS[name]
    osk, refs, queries, answers = kd.oracle_cell(cell)
    for q, (hits, det) in zip(queries, answers):
        n_maps = len(det["mappings"]["qseq"])
        assert len(hits) == cell["hits"], (name, hits)
        assert (n_maps > 0) == cell["maps"], (name, n_maps)
        assert kd.max_seed_hits(osk, cell, q) <= kd.SEED_CAP
    if cell["kind"] != "fragment":
        assert cell["hits"] >= 3
    else:
        k, w, frag = cell["k"], cell["w"], cell["frag"]
        assert (frag < k + w - 1) == (not cell["maps"])
        if cell["maps"]:
            # from k + w - 1 on every fragment holds a window: sketches of one record map
            sizes = set(answers[0][1]["mappings"]["sketch"].tolist())
            assert (sizes == {1} if frag == k + w - 1 else 1 in sizes if frag == k + w else min(sizes) >= 2), sizes
