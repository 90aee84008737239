"""The genome-level screen of the library (fa_screen_signatures / fa_screen_pairs / fa_screen_groups,
pyfastani_amd/csrc/fa_screen.hip.h), restated in plain numpy, and the named cases both test files run.

  signature   np.unique of a genome's hashes, cut at s
  pair        np.union1d cut at s, np.isin in both
  filter      shared * jd >= jn * denom in Python integers
  groups      a union-find that keeps the smaller root

tests/test_screen_inputs.py checks the restatement on the CPU against a second definition with Python sets;
tests/test_gpu_screen.py compares the library with it byte for byte.
"""
import functools

import numpy as np

from pyfastani_amd.screen import SCREEN_DTYPE

MAX_HASH = 0xFFFFFFFF
SIZES = (1, 2, 63, 64, 65, 1000, 4096)


def tile(s):
    """genomes per tile side of the pair kernel: the largest power of two <= 64 with 2 * T * s words in 64 KiB, at least 2
    (the kernel pads a row to the power of two that holds s, which moves none of the thresholds)"""
    t = 64
    while t > 2 and 2 * t * s > 16384:
        t //= 2
    return t


# ---- the restatement -------------------------------------------------------------------------------------------------
def restate_signatures(case):
    """(sig uint32 [n, s], count int32 [n])"""
    s, sbf = case["s"], case["sbf"]
    sig = np.zeros((len(sbf), s), dtype=np.uint32)
    count = np.zeros(len(sbf), dtype=np.int32)
    for g in range(len(sbf)):
        lo, hi = (int(sbf[g - 1]) if g else 0), int(sbf[g])
        mine = np.unique(case["hash"][(case["seq_id"] >= lo) & (case["seq_id"] < hi)])[:s]
        sig[g, : len(mine)], count[g] = mine, len(mine)
    return sig, count


def pair_statistic(a, b, s):
    """(shared, denom) of two ascending distinct arrays"""
    union = np.union1d(a, b)
    denom = min(s, len(union))
    head = union[:denom]
    return int(np.sum(np.isin(head, a) & np.isin(head, b))), denom


def keeps(shared, denom, jn, jd):
    return denom > 0 and int(shared) * int(jd) >= int(jn) * int(denom)


def restate_pairs(case):
    """(records SCREEN_DTYPE sorted by (a, b), (evaluated, kept))"""
    s, out, evaluated = case["s"], [], 0
    sig_a, count_a, sig_b, count_b = case["sig_a"], case["count_a"], case["sig_b"], case["count_b"]
    for a in range(len(count_a)):
        for b in range(a + 1 if case["triangular"] else 0, len(count_b)):
            evaluated += 1
            shared, denom = pair_statistic(sig_a[a, : count_a[a]], sig_b[b, : count_b[b]], s)
            if keeps(shared, denom, case["jn"], case["jd"]):
                out.append((a, b, shared, denom))
    return np.array(out, dtype=SCREEN_DTYPE), (evaluated, len(out))


def restate_groups(records, n):
    """(labels int32 [n], n_groups)"""
    root = list(range(n))

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x
    for r in records:
        x, y = find(int(r["a"])), find(int(r["b"]))
        if x != y:
            root[max(x, y)] = min(x, y)
    labels = np.array([find(g) for g in range(n)], dtype=np.int32)
    return labels, int(np.sum(labels == np.arange(n)))


# ---- signature cases -------------------------------------------------------------------------------------------------
def distinct_hashes(g, n, avoid=()):
    """n distinct uint32 values in random order, none of `avoid`"""
    out = set()
    while len(out) < n:
        out.update(int(v) for v in g.integers(0, MAX_HASH + 1, n - len(out) + 8, dtype=np.uint64))
        out.difference_update(avoid)
        while len(out) > n:
            out.pop()
    return g.permutation(np.array(sorted(out), dtype=np.uint32))


def records_case(genomes, s):
    """genomes: a list of genomes, each a list of contigs, each an array of hashes (possibly empty)"""
    hashes, seq, sbf, contig = [], [], [], 0
    for contigs in genomes:
        for h in contigs:
            hashes.append(np.asarray(h, dtype=np.uint32))
            seq.append(np.full(len(h), contig, dtype=np.int32))
            contig += 1
        sbf.append(contig)
    return {"hash": np.concatenate(hashes) if hashes else np.zeros(0, np.uint32),
            "seq_id": np.concatenate(seq) if seq else np.zeros(0, np.int32), "sbf": np.array(sbf, dtype=np.int32), "s": s}


# what the genomes of mixed(s) are there for, by number
MIXED = {"no_contig_first": 0, "one_record": 1, "fewer_than_s": 2, "exactly_s": 3, "contigs_without_records": 4, "repeated_hash": 5,
         "extreme_hashes": 6, "several_contigs": 7, "no_record_last": 8}


def mixed(s):
    g = np.random.default_rng(1000 + s)
    few = distinct_hashes(g, s // 2)
    exact = distinct_hashes(g, s)
    spread = distinct_hashes(g, 2 * s + 3, avoid=(0, MAX_HASH))
    pieces = np.array_split(distinct_hashes(g, 2 * s + 5), 4)
    genomes = [
        [],
        [np.array([0x9E3779B9], dtype=np.uint32)],
        [g.permutation(np.concatenate([few, few]))],
        [g.permutation(np.concatenate([exact, exact[: s // 3 + 1]]))],
        [np.zeros(0, np.uint32), np.zeros(0, np.uint32)],
        [g.permutation(np.concatenate([np.full(5000, 123456789, dtype=np.uint32), distinct_hashes(g, 3, avoid=(123456789,))]))],
        [g.permutation(np.concatenate([spread, np.array([0, MAX_HASH, 0, MAX_HASH], dtype=np.uint32)]))],
        [pieces[0], pieces[1], np.zeros(0, np.uint32), np.concatenate([pieces[2], pieces[0][:2]]), pieces[3]],
        [np.zeros(0, np.uint32)],
    ]
    return records_case(genomes, s)


def many_genomes(n, s, seed):
    """n genomes of 0 .. 4 s records from a common pool, so that duplicates inside a genome and between genomes occur"""
    g = np.random.default_rng(seed)
    pool = distinct_hashes(g, 2 * s + 10)
    genomes = []
    for i in range(n):
        size = int(g.integers(0, 4 * s + 2)) if i % 7 else 0
        genomes.append(np.array_split(pool[g.integers(0, len(pool), size)], 1 + i % 3))
    return records_case(genomes, s)


@functools.lru_cache(maxsize=None)
def signature_cases():
    out = {f"mixed_s{s}": mixed(s) for s in SIZES}
    out["three_genomes_s64"] = records_case([[distinct_hashes(np.random.default_rng(3), 100)], [], [np.array([7, 7, 9], np.uint32)]], 64)
    out["three_hundred_genomes_s64"] = many_genomes(300, 64, 300)
    out["three_hundred_genomes_s1000"] = many_genomes(300, 1000, 301)
    out["no_records_at_all"] = records_case([[], [np.zeros(0, np.uint32)], []], 5)
    return out


# ---- pair cases ------------------------------------------------------------------------------------------------------
def signature_set(arrays, s):
    """(sig uint32 [n, s], count int32 [n]) of ascending distinct arrays"""
    sig = np.zeros((len(arrays), s), dtype=np.uint32)
    count = np.zeros(len(arrays), dtype=np.int32)
    for i, a in enumerate(arrays):
        a = np.unique(np.asarray(a, dtype=np.uint32))
        assert len(a) <= s
        sig[i, : len(a)], count[i] = a, len(a)
    return sig, count


def pair_case(set_a, set_b, s, triangular, jn=0, jd=1):
    return {"sig_a": set_a[0], "count_a": set_a[1], "sig_b": set_b[0], "count_b": set_b[1], "s": s, "triangular": triangular,
            "jn": jn, "jd": jd}


# the genomes of named_set(s), s >= 8, by number
NAMED = {"full": 0, "full_again": 1, "disjoint_full": 2, "short": 3, "other_short": 4, "empty": 5, "other_empty": 6,
         "shared_late_a": 7, "shared_late_b": 8, "half_shared": 9}


def named_set(s):
    g = np.random.default_rng(50 + s)
    pool = np.sort(distinct_hashes(g, 4 * s, avoid=(0, MAX_HASH)))
    low, high = pool[: 2 * s], pool[2 * s:]                        # every element of `low` is below every element of `high`
    full = low[0::2][:s]
    short, other_short = full[: s // 4], np.concatenate([full[s // 8: s // 4], low[1::2][: s // 8]])
    late = high[-1]
    shared_late_a = np.concatenate([low[0::2][: s - 1], [late]])
    shared_late_b = np.concatenate([low[1::2][: s - 1], [late]])
    half_shared = np.concatenate([full[: s // 2], high[: s - s // 2]])
    return signature_set([full, full, high[:s], short, other_short, [], [], shared_late_a, shared_late_b, half_shared], s)


def random_set(n, s, seed):
    """n signatures drawn from a pool of 3 s hashes: empty, short, full and nearly full ones, all sharing with each other"""
    pool = distinct_hashes(np.random.default_rng(s), 3 * s + 2)     # one pool per s: sets of different seeds share too
    g = np.random.default_rng(seed)
    sizes = [0, 1, s, max(s - 1, 0), s // 2, s]
    return signature_set([g.choice(pool, size=min(sizes[(i + seed) % len(sizes)], len(pool)), replace=False) for i in range(n)], s)


def boundary_set():
    """s = 7: (0, 1) has shared / denom = 3 / 7, (0, 2) 7 / 7, (1, 2) 3 / 7"""
    return signature_set([[1, 2, 3, 4, 5, 6, 7], [1, 2, 3, 8, 9, 10, 11], [1, 2, 3, 4, 5, 6, 7]], 7)


@functools.lru_cache(maxsize=None)
def pair_cases():
    out = {}
    for s in (8, 65, 1000, 4096, 64):
        named = named_set(s)
        out[f"named_s{s}_triangular"] = pair_case(named, named, s, True)
        out[f"named_s{s}_rectangular"] = pair_case(named, named, s, False)
    out["named_s64_half_kept"] = pair_case(named, named, 64, True, jn=1, jd=4)
    for s in (1, 2):
        small = signature_set([[5], [5], [6], [], [0], [MAX_HASH], [0, MAX_HASH][:s], []], s)
        out[f"small_s{s}_triangular"] = pair_case(small, small, s, True)
        out[f"small_s{s}_rectangular"] = pair_case(small, small, s, False)
    for s in (64, 1000, 4096):                                     # tiles of 64, 8 and 2 genomes a side
        t = tile(s)
        sets = {n: random_set(n, s, 7 * s + n) for n in (t - 1, t, t + 1)}
        for n_a in sets:
            for n_b in sets:
                out[f"tile_s{s}_{n_a}_x_{n_b}"] = pair_case(sets[n_a], sets[n_b], s, False, jn=1, jd=8)
            out[f"tile_s{s}_{n_a}_triangular"] = pair_case(sets[n_a], sets[n_a], s, True, jn=1, jd=8)
    several = random_set(2 * tile(1000) + 3, 1000, 99)             # more than one tile and more than one workgroup a side
    out["several_tiles_s1000_triangular"] = pair_case(several, several, 1000, True, jn=1, jd=8)
    out["several_tiles_s1000_rectangular"] = pair_case(several, several, 1000, False, jn=1, jd=8)
    wide = random_set(130, 8, 130)                                 # rows of three mask words
    out["three_mask_words_s8"] = pair_case(random_set(3, 8, 3), wide, 8, False, jn=1, jd=8)
    out["three_mask_words_s8_triangular"] = pair_case(wide, wide, 8, True, jn=1, jd=2)
    boundary = boundary_set()
    for label, (jn, jd) in {"met": (3000, 7000), "missed_by_one": (3001, 7000), "all": (0, 1), "only_identical": (1, 1),
                            "wide_met": (3 * 306783378, 7 * 306783378), "wide_missed": (3 * 306783378 + 1, 7 * 306783378)}.items():
        out[f"boundary_{label}"] = pair_case(boundary, boundary, 7, True, jn=jn, jd=jd)
    empty = signature_set([], 16)
    out["no_genomes"] = pair_case(empty, empty, 16, True)
    out["no_genomes_against_some"] = pair_case(empty, random_set(3, 16, 1), 16, False)
    return out


# ---- group cases -----------------------------------------------------------------------------------------------------
def edge_records(edges):
    out = np.zeros(len(edges), dtype=SCREEN_DTYPE)
    for i, (a, b) in enumerate(edges):
        out[i] = (a, b, 1, 1)
    return out


@functools.lru_cache(maxsize=None)
def group_cases():
    """name -> (records, n, labels expected by hand, groups)"""
    chain = [(i, i + 1) for i in range(0, 299)][::-1]
    return {
        "chain": (edge_records(chain), 300, [0] * 300, 1),
        "star": (edge_records([(2, 5), (1, 5), (5, 9), (0, 5), (5, 6)]), 10, [0, 0, 0, 3, 4, 0, 0, 7, 8, 0], 5),
        "two_components": (edge_records([(4, 5), (0, 2), (2, 3), (1, 5), (1, 4)]), 6, [0, 1, 0, 0, 1, 1], 2),
        "no_edges": (edge_records([]), 7, list(range(7)), 7),
    }


# ---- the end-to-end fixture ------------------------------------------------------------------------------------------
FAMILY_SEED = 500                  # (chosen on the CPU: tests/test_screen_inputs.py says what it has to give)
FAMILIES, MEMBERS, FAMILY_LENGTH = 3, 4, 100_000


@functools.lru_cache(maxsize=None)
def family_genomes():
    """three families of four 100 kb genomes: a random ancestor each, members mutated at the first four DIVERGENCES"""
    from pyfastani_amd import synthetic as syn
    genomes = []
    for f in range(FAMILIES):
        genomes += syn.family(FAMILY_SEED + f, MEMBERS, FAMILY_LENGTH)[1]
    return genomes
