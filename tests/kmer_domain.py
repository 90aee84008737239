"""Inputs of the k-mer-size domain tests: the k at which the hashing, the staging and the length arithmetic change their
behaviour, one window per form of K1, the sequences that put them under load, and the end-to-end cells with their generators.
Shared by tests/test_kmer_domain_inputs.py (oracle only, no GPU), tests/test_gpu_kmer_domain.py and
scripts/fuzz_parity.py --kmers.  Nothing here touches the GPU but `sketch_pair`, which only the GPU test calls."""
import os
import warnings

import numpy as np

from oracle.oracle import OracleSketch
from pyfastani_amd import synthetic as syn

TILE = 1024                               # fa_sketch.hip.h: the positions of a full tile

# The critical k (hash_codes<0> / hash_bytes split a k-mer into k >> 4 blocks of 16 bytes and a tail of k & 15):
KS = [
    1, 2, 3, 4, 5, 6,           # the low end of the accepted range: no block, 4^k k-mers (equal hashes everywhere); at even
                                # k palindromes (forward hash == reverse hash) leave positions without a k-mer
    7, 8, 9, 10,                # tail remainders 7 / 8 / 9: the tail's second lane is masked in from rem > 8 on
    13, 15, 17,                 # the neighbours of the premixed k = 14 / 16 (generic form inside k_sketch_fast);
                                # remainder 15, zero blocks; remainder 1, one block
    20, 22,                     # the neighbours of the premixed k = 21
    24, 25, 31,                 # one block with remainders 8 / 9 / 15
    47, 48, 49,                 # two / three blocks: remainders 15 / 0 / 1
    63, 64, 65,                 # many blocks, remainders 15 / 0 / 1
    127, 128, 129, 255, 256, 257,
    1000,                       # remainder 8 with 62 blocks
    1023, 1024, 1025,           # k around TILE: from k > 1024 the k - 1 extra bases staged outgrow the tile itself
    2047, 2048,                 # the high end of the accepted range (remainders 15 / 0)
]
# One window per form of K1: 1 and 2 take the 64-bit window minimum of k_sketch_tiles; 4, 24 and 64 k_sketch_fast; 65 and
# 385 the 32-bit minimum of k_sketch_tiles (385: the tile length at its floor of 256); 1001 the 64-bit one again.
WS = [1, 2, 4, 24, 64, 65, 385, 1001]
DEFINITION_KS = [1, 2, 4, 8, 9, 15, 48, 257, 2048]
DEFINITION_WS = [1, 4, 64, 65, 1001]
PROTEIN_KS = [1, 2, 8, 9, 15, 16, 17, 31, 32, 33, 64, 2048]
AMINO = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
SEED_CAP = 8192                           # seed hits of one fragment inside one reference contig that every cell stays below


def k1_tile_len(w):
    """Positions per tile of reference sketching (fa_sketch.hip.h: k1_tile_len; FA_K1_TILE overrides it).  A restatement:
    nothing reads the header."""
    forced = int(os.environ.get("FA_K1_TILE", "0") or 0)
    if 256 <= forced <= TILE and forced % 4 == 0:
        return forced
    return max(256, (TILE - (2 * w - 2)) & ~3)


# ----------------------------------------------------------------------------------------------------------------
# MurmurHash3_x64_128, seed 42, low 32 bits of the sum's low half -- from the published algorithm (Appleby, smhasher), in
# plain Python integers; `murmur3_positions` is the same over every k-mer of a sequence at once (numpy, modulo 2^64)
# ----------------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1
_C1, _C2 = 0x87C37B91114253D5, 0x4CF5AD432745937F


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M64


def _fmix(x):
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & _M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & _M64
    x ^= x >> 33
    return x


def murmur3_32(data, seed=42):
    data = bytes(data)
    n = len(data)
    h1 = h2 = seed
    for b in range(n // 16):
        k1 = int.from_bytes(data[16 * b: 16 * b + 8], "little")
        k2 = int.from_bytes(data[16 * b + 8: 16 * b + 16], "little")
        k1 = (k1 * _C1) & _M64; k1 = _rotl(k1, 31); k1 = (k1 * _C2) & _M64; h1 ^= k1
        h1 = _rotl(h1, 27); h1 = (h1 + h2) & _M64; h1 = (h1 * 5 + 0x52DCE729) & _M64
        k2 = (k2 * _C2) & _M64; k2 = _rotl(k2, 33); k2 = (k2 * _C1) & _M64; h2 ^= k2
        h2 = _rotl(h2, 31); h2 = (h2 + h1) & _M64; h2 = (h2 * 5 + 0x38495AB5) & _M64
    tail = data[n // 16 * 16:]
    if len(tail) > 8:
        k2 = int.from_bytes(tail[8:], "little")
        k2 = (k2 * _C2) & _M64; k2 = _rotl(k2, 33); k2 = (k2 * _C1) & _M64; h2 ^= k2
    if len(tail) > 0:
        k1 = int.from_bytes(tail[:8], "little")
        k1 = (k1 * _C1) & _M64; k1 = _rotl(k1, 31); k1 = (k1 * _C2) & _M64; h1 ^= k1
    h1 ^= n; h2 ^= n
    h1 = (h1 + h2) & _M64; h2 = (h2 + h1) & _M64
    h1 = _fmix(h1); h2 = _fmix(h2)
    h1 = (h1 + h2) & _M64
    return h1 & 0xFFFFFFFF


def murmur3_positions(seq, k, seed=42):
    """murmur3_32(seq[i:i + k]) for every i, as a uint32 array (tests/test_kmer_domain_inputs.py holds it to murmur3_32)."""
    a = np.frombuffer(bytes(seq), dtype=np.uint8)
    n = len(a) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint32)
    u = np.uint64
    pad = np.concatenate([a, np.zeros(16, np.uint8)]).astype(u)
    word = np.zeros(len(a) + 9, u)                     # word[i] = the eight bytes from i on, little-end first
    for j in range(8):
        word |= pad[j: j + len(word)] << u(8 * j)
    rot = lambda x, r: (x << u(r)) | (x >> u(64 - r))  # noqa: E731
    c1, c2 = u(_C1), u(_C2)
    h1 = np.full(n, seed, u)
    h2 = np.full(n, seed, u)
    at = np.arange(n)
    with np.errstate(over="ignore"):
        for b in range(k // 16):
            k1, k2 = word[at + 16 * b], word[at + 16 * b + 8]
            h1 ^= rot(k1 * c1, 31) * c2
            h1 = (rot(h1, 27) + h2) * u(5) + u(0x52DCE729)
            h2 ^= rot(k2 * c2, 33) * c1
            h2 = (rot(h2, 31) + h1) * u(5) + u(0x38495AB5)
        rem, t0 = k % 16, k // 16 * 16
        mask = lambda m: u(_M64 if m >= 8 else (1 << (8 * m)) - 1)  # noqa: E731
        if rem > 8:
            h2 ^= rot((word[at + t0 + 8] & mask(rem - 8)) * c2, 33) * c1
        if rem > 0:
            h1 ^= rot((word[at + t0] & mask(min(rem, 8))) * c1, 31) * c2
        h1 ^= u(k); h2 ^= u(k)
        h1 = h1 + h2; h2 = h2 + h1
        for m in (u(0xFF51AFD7ED558CCD), u(0xC4CEB9FE1A85EC53)):
            h1 ^= h1 >> u(33); h1 = h1 * m
            h2 ^= h2 >> u(33); h2 = h2 * m
        h1 ^= h1 >> u(33); h2 ^= h2 >> u(33)
        return ((h1 + h2) & u(0xFFFFFFFF)).astype(np.uint32)


_RC = bytes.maketrans(b"ACGT", b"TGCA")


class HashOf:
    """murmur3_32 of every k-mer of `seq` and of its reverse complement, computed at once and looked up by the k-mer: what
    `check_winnowing` of the window test calls once per position (two million bytes of Python hashing at k = 2048)."""

    def __init__(self, seq, k):
        self.table = {}
        for s in (bytes(seq), bytes(seq).translate(_RC)[::-1]):
            for i, h in enumerate(murmur3_positions(s, k).tolist()):
                self.table[s[i:i + k]] = h

    def __call__(self, kmer):
        return self.table[bytes(kmer)]


# ----------------------------------------------------------------------------------------------------------------
# streams
# ----------------------------------------------------------------------------------------------------------------
def rnd(g, n):
    return bytes(syn.to_ascii(syn.random_codes(g, n)))


def with_repeats(g, n, w):
    # tests/test_gpu_window_domain.py: with_repeats -- one k-mer occurring again within and beyond a window
    c = syn.random_codes(g, n)
    unit = syn.random_codes(g, int(g.integers(20, 120)))
    for _ in range(6):
        p = int(g.integers(0, max(1, n - 400)))
        c[p:p + len(unit)] = unit[: n - p]
    span = max(40, min(w, n // 4))
    p = int(g.integers(0, max(1, n - 2 * span)))
    c[p + span: p + 2 * span] = c[p: p + span]
    return bytes(syn.to_ascii(c))


def full_length(k, w):
    """What a case that is meant to yield records holds at least: three tiles, the halo and the k - 1 bases behind them."""
    return 3 * k1_tile_len(w) + 2 * w + k


def stream_cases(k, w, g):
    """The cases of tests/test_gpu_window_domain.py: stream_cases, lengthened to `full_length` where they are meant to yield
    records, plus: two letters only; AT and ACGT repeats (at even k every k-mer of the first is its own reverse complement, and every second or
    fourth one of the second: positions without a k-mer and without any N); one stretch of exactly k, k + w - 2, k + w - 1 and k + w bases between two runs of N (a k-mer
    of N alone is its own reverse complement, so nothing outside the stretch and its flanks holds a k-mer); IUPAC and
    lower-case bytes (the byte path, k_sketch_tiles<0, true>)."""
    tl, full = k1_tile_len(w), full_length(k, w)
    half = max(900, (full + 1) // 2)
    cases = {
        "random": rnd(g, max(6000, full)),
        "two_letters": bytes(np.frombuffer(b"AC", np.uint8)[g.integers(0, 2, max(4000, full))]),
        "ATGC_repeat": b"ATGC" * (max(3200, full) // 4 + 1),
        "ACGT_repeat": b"ACGT" * (max(3200, full) // 4 + 1),
        "polyA": b"A" * max(2 * w + k + 300, full),
        "AT_repeat": b"AT" * (max(3000, full) // 2 + 1),
        "N_runs_longer_than_w": rnd(g, max(2500, full)) + b"N" * (w + 7) + rnd(g, max(1500, w + k + 300)) + b"N" * (2 * w + 1)
                                + rnd(g, w + k + 5),
        "iupac_lower": rnd(g, half) + b"nnRYKMBVDHSWU" + rnd(g, half).lower(),
        "shorter_than_k": rnd(g, k - 1),
        "len_w_plus_k_minus_2": rnd(g, w + k - 2),
        "len_w_plus_k_minus_1": rnd(g, w + k - 1),
        "len_w_plus_k": rnd(g, w + k),
        "palindromes": (rnd(g, 40) + b"ACGT" * 10 + b"GAATTC" * 20) * max(8, full // 200 + 1),
        "repeats": with_repeats(g, max(5000, full), w),
    }
    for name, n in (("k", k), ("k_w_minus_2", k + w - 2), ("k_w_minus_1", k + w - 1), ("k_w", k + w)):
        cases[f"stretch_{name}"] = b"N" * (k + w + 3) + rnd(g, n) + b"N" * (k + w + 1)
    for j in (1, 2, 3):
        for d in (-1, 0, 1):
            cases[f"tiles_{j}{d:+d}"] = rnd(g, j * tl + 2 * w + k + d)
    return cases


# cases that yield records at every (k, w) (the others may not: palindromes at even k, a single window of them at k = 2)
YIELDING = ("random", "two_letters", "polyA", "N_runs_longer_than_w", "iupac_lower", "repeats", "tiles_1+0", "tiles_3+1")


def definition_cases(k, w, g):
    """Three pure-ACGT sequences for the check by definition: three tiles, planted repeats, exactly one window."""
    return [rnd(g, full_length(k, w)), with_repeats(g, max(4000, 2 * w + k + 600), w), rnd(g, w + k - 1)]


def protein_cases(k, g):
    res = lambda n: bytes(AMINO[g.integers(0, 20, n)])  # noqa: E731
    return {"random": res(max(5000, k + 3000)), "k_minus_1": res(k - 1), "k": res(k), "k_plus_1": res(k + 1)}


# ----------------------------------------------------------------------------------------------------------------
# sketches with an explicit (k, w)
# ----------------------------------------------------------------------------------------------------------------
def oracle_sketch(k, w, fragment_length=3000, minimum_fraction=0.2):
    osk = OracleSketch(k=k, fragment_length=fragment_length, minimum_fraction=minimum_fraction, window=w)
    assert osk.window_size == w and osk.k == k
    return osk


def sketch_pair(k, w, fragment_length=3000, minimum_fraction=0.2, rules=None):
    """(pf.Sketch, OracleSketch) with exactly these parameters.  The Python constructor only ever takes the recommended
    window (the fragment length itself from about k = 22 on, where nothing maps); `Sketch.__setstate__` makes a new native
    sketch from the parameters of its state, so the state of an empty sketch with the parameters edited gives any (k, w)."""
    import pyfastani_amd as pf
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk = pf.Sketch()
    state = sk.__getstate__()
    assert state["sketch"]["minimizers"]["length"] == 0 and not state["names"]
    state["parameters"].update(kmerSize=k, windowSize=w, minReadLength=fragment_length, minFraction=minimum_fraction)
    if rules is not None:
        state["rules"] = rules._asdict()
    sk.__setstate__(state)
    assert (sk.k, sk.window_size, sk.fragment_length) == (k, w, fragment_length)
    return sk, oracle_sketch(k, w, fragment_length, minimum_fraction)


# ----------------------------------------------------------------------------------------------------------------
# end-to-end cells
# ----------------------------------------------------------------------------------------------------------------
def _cell(kind, k, w, frag=3000, **kw):
    return dict(kind=kind, k=k, w=w, frag=frag, minfrac=0.2, hits=3, maps=True, **kw)


SMALL = [(1, 4), (2, 4), (3, 4), (4, 4), (5, 8), (6, 8), (7, 12)]
MIDDLE = [(8, 17), (9, 27), (13, 37), (15, 30), (17, 33), (20, 24), (22, 24), (24, 24), (25, 24), (31, 24), (47, 24), (48, 100),
          (49, 24), (64, 24), (100, 24)]
LARGE = [(255, 24, 3000), (256, 24, 3000), (257, 24, 3000), (1000, 24, 3000), (2047, 24, 3000), (2048, 24, 3000), (2048, 4, 2100),
         (2048, 64, 5000), (2048, 65, 5000), (2048, 1001, 5000)]
FRAGMENT_KW = [(300, 24), (2048, 24)]
FRAGMENT_LENGTHS = {"k-1": lambda k, w: k - 1, "k": lambda k, w: k, "k+w-2": lambda k, w: k + w - 2,
                    "k+w-1": lambda k, w: k + w - 1, "k+w": lambda k, w: k + w, "k+2w": lambda k, w: k + 2 * w}
MAPS_NOTHING = ("k-1", "k", "k+w-2")     # no k-mer, no window, no window: nothing maps, on either side, without an error

CELLS = {}
for _k, _w in SMALL:
    # with 4^k k-mers the unrelated genome shares every hash: it is a hit too
    CELLS[f"small-k{_k}-w{_w}"] = dict(_cell("small", _k, _w), hits=4)
for _k, _w in MIDDLE:
    CELLS[f"middle-k{_k}-w{_w}"] = _cell("middle", _k, _w)
for _k, _w, _f in LARGE:
    CELLS[f"large-k{_k}-w{_w}-f{_f}"] = _cell("large", _k, _w, _f)
for _k, _w in FRAGMENT_KW:
    for _name, _fn in FRAGMENT_LENGTHS.items():
        for _contigs in (1, 2):
            nothing = _name in MAPS_NOTHING
            CELLS[f"fragment-k{_k}-w{_w}-{_name}-c{_contigs}"] = dict(
                _cell("fragment", _k, _w, _fn(_k, _w), contigs=_contigs), minfrac=0.0, hits=0 if nothing else 2, maps=not nothing)
for _i, _c in enumerate(CELLS.values()):
    _c["seed"] = 9600 + _i


def cut_in(seq, n):
    """`seq` as n contigs of equal length (the last takes the remainder)."""
    step = len(seq) // n
    return [seq[i * step: (i + 1) * step if i < n - 1 else len(seq)] for i in range(n)]


def build_cell(cell):
    """(refs, queries) of a cell, as lists of contigs (bytes); queries[0] is the query of the one-query road, all of them the
    resident batch.
    small / middle: the genomes of tests/test_gpu_window_domain.py: test_window_extremes_end_to_end at 12 kb / 40 kb: relatives
    of one ancestor at 0.001, 0.004 and 0.002 (the last in three contigs), a random genome of half the length, a draft query
    at 0.003 and a second one at 0.001.
    large: an exact copy of the ancestor, mutants at 0.0001 and 0.0003, a random genome; the queries at 0.0001, whole and as a
    draft of two contigs (at 0.3 % nothing survives a 1000-mer).
    fragment: a 20 kb genome and a mutant at 0.0001 as references, the genome itself and a second mutant as queries, every
    genome in one contig or cut in two."""
    g = syn.rng(cell["seed"])
    asc = lambda codes: bytes(syn.to_ascii(codes))  # noqa: E731
    split = lambda codes, n: [bytes(c) for c in syn.split_contigs(g, syn.to_ascii(codes), n)]  # noqa: E731
    kind = cell["kind"]
    if kind in ("small", "middle"):
        length = 12_000 if kind == "small" else 40_000
        anc = syn.random_codes(g, length)
        refs = [[asc(syn.mutate_codes(g, anc, d))] for d in (0.001, 0.004)]
        refs.append(split(syn.mutate_codes(g, anc, 0.002), 3))
        refs.append([asc(syn.random_codes(g, length // 2))])
        queries = [split(syn.mutate_codes(g, anc, 0.003), 4), [asc(syn.mutate_codes(g, anc, 0.001))]]
    elif kind == "large":
        anc = syn.random_codes(g, 40_000)
        refs = [[asc(anc)], [asc(syn.mutate_codes(g, anc, 0.0001))], [asc(syn.mutate_codes(g, anc, 0.0003))],
                [asc(syn.random_codes(g, 40_000))]]
        queries = [[asc(syn.mutate_codes(g, anc, 0.0001))], split(syn.mutate_codes(g, anc, 0.0001), 2)]
    else:
        anc = syn.random_codes(g, 20_000)
        n = cell["contigs"]
        refs = [cut_in(asc(anc), n), cut_in(asc(syn.mutate_codes(g, anc, 0.0001)), n)]
        queries = [cut_in(asc(anc), n), cut_in(asc(syn.mutate_codes(g, anc, 0.0001)), n)]
    return refs, queries


def oracle_cell(cell, threads=8):
    """The oracle's answers of a cell: the index, and per query (hits, details)."""
    refs, queries = build_cell(cell)
    osk = oracle_sketch(cell["k"], cell["w"], cell["frag"], cell["minfrac"])
    for i, r in enumerate(refs):
        osk.add_draft(f"ref{i}", r)
    osk.index()
    return osk, refs, queries, [osk.query_draft(q, threads=threads, details=True) for q in queries]


def max_seed_hits(osk, cell, query):
    """The most seed hits a fragment of `query` gathers inside one reference contig: the records of the contig whose hash is
    among the fragment's minimizers, counted from the oracle's minimizers."""
    k, w, frag = cell["k"], cell["w"], cell["frag"]
    rh, rs, _ = osk.minimizers()
    worst = 0
    for c in query:
        if len(c) < min(w, k, frag):
            continue
        for i in range(len(c) // frag):
            qh, _ = osk.sketch_sequence(c[i * frag:(i + 1) * frag])
            on = rs[np.isin(rh, np.unique(qh))]
            if len(on):
                worst = max(worst, int(np.bincount(on).max()))
    return worst
