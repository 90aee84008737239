"""The sketch and mapping kernels across the whole window-size range -- MI355X only.

Nearly every kernel form is picked by the window w, and through w by the sketch size s ~ 2 fragment / (w + 1):
k_sketch_fast serves 4 <= w <= 64 (SKF_MIN_W, SKF_MAX_W); k_sketch_tiles takes its 32-bit window minimum for 3 <= w <= 1000
(levels = floor(log2 w)) and the 64-bit one outside; k1_tile_len(w) stops shrinking at 256 positions from w = 385 on, where
the halo 2w - 2 outgrows the tile; the 16- / 32-bit slide events, the k_l1 size classes and the speculated capacities follow s.
The minimizer streams are checked at every one of those boundaries (and the powers of two of `levels`) against the oracle AND
against two properties of winnowing that hold whatever the tie rule; the end-to-end cells run the recommended windows of the
extreme identities (w = 2 .. 2000), p-values and reference sizes, against the oracle mapping for mapping, and assert the form
that ran."""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import pyfastani_amd as pf
from oracle.oracle import OracleSketch, murmur_hash
from pyfastani_amd import _lib, diagnostics, synthetic as syn
from pyfastani_amd._lib import lib, check
from test_gpu_parity import gpu_mappings, hit_tuples, oracle_mappings, quiet_sketch, run_both

pytestmark = pytest.mark.gpu

# every form boundary of K1 (3 / 4 / 64 / 1000 / 385 ...) and the powers of two of `levels`
WINDOWS = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 384, 385, 386, 511, 512, 513, 1000, 1001, 1023, 1024, 1025,
           2000, 2049]
KS = [11, 14, 16, 21, 32, 33]
DEFINITION_WINDOWS = [1, 2, 3, 4, 64, 65, 385, 1000, 1001, 2049]
TILE = 1024
FUSED_CELLS = {(14, 12), (14, 37), (14, 50), (16, 13), (16, 24), (16, 40), (21, 15), (21, 25)}   # FA_KW_CELLS, fa_k1.hip.h


def k1_tile_len(w):
    # fa_sketch.hip.h: positions per tile of reference sketching (FA_K1_TILE overrides it)
    forced = int(os.environ.get("FA_K1_TILE", "0") or 0)
    if 256 <= forced <= TILE and forced % 4 == 0:
        return forced
    return max(256, (TILE - (2 * w - 2)) & ~3)


def params_for(k, w):
    return _lib.Params(k, w, 3000, 4, 0.2, 80.0, 1e-3, 5_000_000)


def gpu_stream(p, seq):
    cap = max(len(seq), 1)
    h = np.empty(cap, np.uint32)
    wp = np.empty(cap, np.int32)
    n = C.c_int64(0)
    check(lib.fa_debug_sketch_sequence(C.byref(p), seq, len(seq), 1, h.ctypes.data, wp.ctypes.data, cap, C.byref(n)))
    assert n.value <= cap
    return h[: n.value], wp[: n.value]


def rnd(g, n):
    return bytes(syn.to_ascii(syn.random_codes(g, n)))


def with_repeats(g, n, w):
    # pure ACGT with planted repeats: one k-mer occurring again within and beyond a window (equal hashes: ties)
    c = syn.random_codes(g, n)
    unit = syn.random_codes(g, int(g.integers(20, 120)))
    for _ in range(6):
        p = int(g.integers(0, max(1, n - 400)))
        c[p:p + len(unit)] = unit[: n - p]
    span = max(40, min(w, n // 4))
    p = int(g.integers(0, max(1, n - 2 * span)))
    c[p + span: p + 2 * span] = c[p: p + span]
    return bytes(syn.to_ascii(c))


def stream_cases(k, w, g):
    tl = k1_tile_len(w)
    cases = {
        "random": rnd(g, 6000),
        "ATGC_repeat": b"ATGC" * 800,
        "polyA": b"A" * (2 * w + k + 300),
        "AT_repeat": b"AT" * 1500,
        "N_runs_longer_than_w": rnd(g, 2500) + b"N" * (w + 7) + rnd(g, 1500) + b"N" * (2 * w + 1) + rnd(g, w + k + 5),
        "iupac_lower": rnd(g, 900) + b"nnRYKMBVDHSWU" + rnd(g, 900).lower(),
        "shorter_than_k": rnd(g, k - 1),
        "len_w_plus_k_minus_2": rnd(g, w + k - 2),
        "len_w_plus_k_minus_1": rnd(g, w + k - 1),
        "len_w_plus_k": rnd(g, w + k),
        "palindromes": (rnd(g, 40) + b"ACGT" * 10 + b"GAATTC" * 20) * 8,
        "repeats": with_repeats(g, 5000, w),
    }
    for j in (1, 2, 3):
        for d in (-1, 0, 1):
            cases[f"tiles_{j}{d:+d}"] = rnd(g, j * tl + 2 * w + k + d)
    return cases


@pytest.mark.parametrize("w", WINDOWS)
def test_window_domain_streams(w):
    g = syn.rng(7000 + w)
    for k in KS:
        p, osk = params_for(k, w), OracleSketch(k=k, window=w)
        assert osk.window_size == w
        for name, seq in stream_cases(k, w, g).items():
            gh, gw = gpu_stream(p, seq)
            oh, ow = osk.sketch_sequence(seq)
            assert np.array_equal(gh, oh) and np.array_equal(gw, ow), f"w={w} k={k} {name}: gpu {len(gh)} records, oracle {len(oh)}"


@pytest.mark.parametrize("env", [{"FA_K1_GENERAL": "1"}, {"FA_K1_TILE": "1024"}], ids=["general", "full-tile"])
def test_window_domain_streams_through_the_other_forms(env):
    # every tile through the 64-bit window minimum / reference tiles of the full 1 024 positions (the halo then always fits
    # in front of a whole tile): the same streams, against the oracle and by definition, in a child process (the knobs are
    # read once per process)
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                          "-k", "test_window_domain_streams and not other_forms"],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    want = len(WINDOWS) + len(DEFINITION_WINDOWS)
    assert res.returncode == 0 and f"{want} passed" in res.stdout, res.stdout[-3000:] + res.stderr[-2000:]


# ----------------------------------------------------------------------------------------------------------------
# winnowing by definition, independent of the oracle
# ----------------------------------------------------------------------------------------------------------------
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def canonical_hashes(seq, k):
    """(hash, valid) per k-mer position of a pure-ACGT sequence: min(forward, reverse complement) of the 32-bit MurmurHash3
    (oracle.murmur_hash, pinned to independent vectors by tests/test_oracle_golden.py); a k-mer whose hash equals that of its
    reverse complement (a palindrome) is skipped by the reference and the kernels alike (_fastani.pyx:202) -- not valid."""
    n = len(seq) - k + 1
    h = np.zeros(max(n, 0), np.uint64)
    valid = np.zeros(max(n, 0), bool)
    rc = seq.translate(_RC)[::-1]
    L = len(seq)
    for i in range(n):
        hf, hb = murmur_hash(seq[i:i + k]), murmur_hash(rc[L - i - k: L - i])
        if hf != hb:
            h[i], valid[i] = min(hf, hb), True
    return h, valid


def sliding_min(a, w):
    # out[i] = min(a[i : i + w]) for i = 0 .. len(a) - w, by doubling
    span, t = 1, a
    while 2 * span <= w:
        t = np.minimum(t[:-span], t[span:])
        span *= 2
    n = len(a) - w + 1
    return np.minimum(t[:n], t[w - span: w - span + n])


def check_winnowing(seq, k, w, hashes, wpos):
    """The window that ends at position i covers the k-mer positions [i - w + 1, i]; the first full window ends at w - 1
    (the start of a sequence: no record before it), the last at len - k (its end).  A record (hash, wpos) was emitted when
    the window [wpos, wpos + w - 1] was read, which happens only at a valid end position.  Then:
      (1) every emitted record is the minimum of the window it was emitted for (a window that contains it);
      (2) at every valid end position i, the last record emitted up to i holds the minimum of window i, and was emitted
          for a window that overlaps it: the minimum of every full window is emitted at a position inside that window.
    Both hold for any rule among equal hashes.  (2)'s second half has one documented exception: a new minimum whose hash
    equals that of the sequence's FIRST record (wpos 0) is not emitted again while that record is the last one
    (_fastani.pyx:216,220)."""
    h, valid = canonical_hashes(seq, k)
    if len(h) < w:
        assert len(hashes) == 0
        return
    big = np.where(valid, h, np.uint64(1) << np.uint64(40))
    wmin = sliding_min(big, w)                                   # wmin[s] = minimum of the window starting at s
    ends = wpos.astype(np.int64) + w - 1
    assert np.all(np.diff(ends) > 0), "records out of order"
    assert np.all(valid[ends]), "a record emitted at a position without a k-mer"
    assert np.array_equal(wmin[wpos].astype(np.uint64), hashes.astype(np.uint64)), "(1) a record is not its window's minimum"
    for i in np.nonzero(valid[w - 1:])[0] + (w - 1):
        r = np.searchsorted(ends, i, side="right") - 1
        assert r >= 0, f"(2) no record by valid position {i}"
        assert int(hashes[r]) == int(wmin[i - w + 1]), f"(2) window ending at {i}: minimum {wmin[i - w + 1]}, last record {hashes[r]}"
        assert ends[r] >= i - w + 1 or (r == 0 and wpos[0] == 0), f"(2) window ending at {i}: its minimum was emitted before it"


@pytest.mark.parametrize("w", DEFINITION_WINDOWS)
def test_window_domain_streams_by_definition(w):
    g = syn.rng(7500 + w)
    for k in (16, 21, 32):
        p = params_for(k, w)
        for seq in (rnd(g, 3 * k1_tile_len(w) + 2 * w + k), with_repeats(g, 4000, w), rnd(g, w + k - 1)):
            gh, gw = gpu_stream(p, seq)
            check_winnowing(seq, k, w, gh, gw)


# ----------------------------------------------------------------------------------------------------------------
# end to end at the extremes of the recommended window
# ----------------------------------------------------------------------------------------------------------------
# (params, expected window): the identities at both ends of the range, the p-value and the reference size
CELLS = [
    ({"k": 16, "fragment_length": 3000, "percentage_identity": 64.5}, 2),
    ({"k": 16, "fragment_length": 3000, "percentage_identity": 67.0}, 3),
    ({"k": 16, "fragment_length": 3000, "percentage_identity": 69.0}, 4),
    ({"k": 16, "fragment_length": 3000, "percentage_identity": 96.0}, 600),
    ({"k": 16, "fragment_length": 3000, "percentage_identity": 99.0}, 1200),
    ({"k": 16, "fragment_length": 3000, "percentage_identity": 100.0}, 1200),
    ({"k": 14, "fragment_length": 1000, "percentage_identity": 68.5}, 2),
    ({"k": 14, "fragment_length": 1000, "percentage_identity": 95.0}, 200),
    ({"k": 14, "fragment_length": 1000, "percentage_identity": 98.0}, 400),
    ({"k": 21, "fragment_length": 5000, "percentage_identity": 68.0}, 2),
    ({"k": 21, "fragment_length": 5000, "percentage_identity": 70.0}, 3),
    ({"k": 21, "fragment_length": 5000, "percentage_identity": 97.0}, 1000),
    ({"k": 21, "fragment_length": 5000, "percentage_identity": 99.0}, 2000),
    ({"k": 16, "fragment_length": 500, "percentage_identity": 96.0}, 100),
    ({"k": 16, "fragment_length": 500, "percentage_identity": 99.0}, 200),
    ({"k": 16, "fragment_length": 3000, "p_value": 1e-1}, 40),
    ({"k": 16, "fragment_length": 3000, "p_value": 1e-12}, 15),
    ({"k": 16, "fragment_length": 3000, "reference_size": 10_000}, 40),
]


@pytest.mark.parametrize("params,w", CELLS, ids=[f"w{w}-" + "-".join(f"{k}{v}" for k, v in p.items()) for p, w in CELLS])
def test_window_extremes_end_to_end(params, w):
    frag = params["fragment_length"]
    g = syn.rng(8000 + w + frag)
    length = max(12 * frag, 40_000)
    anc = syn.random_codes(g, length)
    # genomes within 0.5 % of each other: a high-identity cell that passed on empty output is impossible
    refs = [[syn.to_ascii(syn.mutate_codes(g, anc, d))] for d in (0.001, 0.004)]
    refs.append(syn.split_contigs(g, syn.to_ascii(syn.mutate_codes(g, anc, 0.002)), 3))
    refs.append([syn.to_ascii(syn.random_codes(g, length // 2))])
    query = syn.split_contigs(g, syn.to_ascii(syn.mutate_codes(g, anc, 0.003)), 4)           # a draft query
    mapper, hits, ohits, det = run_both(params, refs, query, threads=8)
    assert mapper.window_size == w
    assert gpu_mappings(mapper) == oracle_mappings(det)
    assert hit_tuples(hits) == ohits
    assert len(ohits) >= 3, ohits
    spec, ms = diagnostics.spec(mapper), diagnostics.timings(mapper)
    k, s = params["k"], 2 * frag // (w + 1)
    # the forms: 32-bit slide events for the sketches of hundreds of records and more (the bound must hold slot = rank + 1 in
    # 9 bits); the 512-thread k_l1 classes where fragments hold more than 4 096 seed hits (three relatives x ~2 000-3 300
    # minimizers at w = 2); one 256-thread class and no pre-filter at the tiny sketches; the one-launch sketch stage
    # (k_query_fused) only in the compiled (k, w) cells -- never beyond w = 1000, where K1 takes the general path
    if w <= 4:
        assert spec.f_wide == 1, spec
    if s <= 100:
        assert spec.f_wide == 0, spec
    if w == 2 and frag >= 3000:
        assert 512 in (spec.l1_t0, spec.l1_t1, spec.l1_t2), spec
    if s <= 10:
        assert spec.n_l1 == 1 and spec.l1_t0 == 256 and spec.f_prefilter == 0, spec
    assert spec.f_prefilter == 0, spec
    if (k, w) not in FUSED_CELLS:
        assert ms.fused == 0 and ms.unfused > 0, ms
    # the same genomes as one resident batch
    sk, osk = quiet_sketch(pf.Sketch, **params), quiet_sketch(OracleSketch, **params)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, r in enumerate(refs):
            sk.add_draft(f"ref{i}", r)
            osk.add_draft(f"ref{i}", r)
        batch_mapper = sk.index()
        osk.index()
        queries = [query, [syn.to_ascii(syn.mutate_codes(g, anc, 0.001))]]
        got = [hit_tuples(h) for h in batch_mapper.upload_genomes(queries).query()]
    want = [osk.query_draft(q, threads=8) for q in queries]
    assert got == want and all(len(x) >= 3 for x in want)


def test_window_equal_to_fragment_maps_nothing():
    # (k = 21, fragment 1000) at the default identity: the recommended window is the fragment itself, no fragment holds a
    # full window, nothing maps -- the one documented empty cell
    g = syn.rng(8999)
    anc = syn.random_codes(g, 40_000)
    refs = [[syn.to_ascii(syn.mutate_codes(g, anc, 0.002))]]
    mapper, hits, ohits, det = run_both({"k": 21, "fragment_length": 1000}, refs, [syn.to_ascii(anc)])
    assert mapper.window_size == 1000 and hits == [] and ohits == []
