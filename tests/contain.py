"""The containment road of the screen (fa_screen_contents / fa_screen_contained, pyfastani_amd/csrc/fa_contain.hip.h),
restated in plain numpy, and the named cases both test files run.

  contents    np.unique over (hash, genome)
  statistic   np.isin of the directory's hashes in the signature, counted per genome
  filter      shared * cd >= cn * denom in Python integers
  visited     the entries (x, b) with x in the signature, summed over the signatures: the sum of every pair's shared

tests/test_contain_inputs.py checks the restatement on the CPU against a second definition with Python sets;
tests/test_gpu_contain.py compares the library with it byte for byte.
"""
import ctypes as C
import functools

import numpy as np

import screen as sc
from pyfastani_amd import _lib
from pyfastani_amd.screen import SCREEN_DTYPE

MAX_HASH = sc.MAX_HASH
SIZES = sc.SIZES


def slice_size():
    """references per workgroup slice of the counting kernel, as the library says (host only)"""
    out = C.c_int32(0)
    assert _lib.lib.fa_screen_contain_slice(C.byref(out)) == _lib.FA_OK
    return out.value


# ---- the restatement -------------------------------------------------------------------------------------------------
def restate_contents(case):
    """(ent_hash uint32 [m], ent_genome int32 [m]) of a records case of tests/screen.py (its "s" plays no part)"""
    genome = np.searchsorted(case["sbf"], case["seq_id"], side="right").astype(np.uint64)       # the first g with sbf[g] > contig
    keys = np.unique(case["hash"].astype(np.uint64) << np.uint64(32) | genome)
    return (keys >> np.uint64(32)).astype(np.uint32), (keys & np.uint64(MAX_HASH)).astype(np.int32)


def keeps(shared, denom, cn, cd):
    return denom > 0 and int(shared) * int(cd) >= int(cn) * int(denom)


def restate_contained(case):
    """(records SCREEN_DTYPE sorted by (a, b), (evaluated, kept, visited))"""
    n_a, n_b, out, visited = len(case["count"]), case["n_b"], [], 0
    for a in range(n_a):
        mine = case["sig"][a, : case["count"][a]]
        denom = len(mine)
        shared = np.bincount(case["ent_genome"][np.isin(case["ent_hash"], mine)], minlength=n_b) if n_b else np.zeros(0, np.int64)
        visited += int(shared.sum())
        for b in range(n_b):
            if keeps(shared[b], denom, case["cn"], case["cd"]):
                out.append((a, b, int(shared[b]), denom))
    return np.array(out, dtype=SCREEN_DTYPE), (n_a * n_b, len(out), visited)


# ---- cases -----------------------------------------------------------------------------------------------------------
def directory(references):
    """(ent_hash, ent_genome) of a list of hash arrays, one per reference genome (duplicates and order do not matter)"""
    genomes = [[np.asarray(r, dtype=np.uint32)] for r in references]
    return restate_contents(sc.records_case(genomes, 1)) if genomes else (np.zeros(0, np.uint32), np.zeros(0, np.int32))


def contain_case(signature_set, references, s, cn=0, cd=1):
    ent_hash, ent_genome = directory(references)
    return {"sig": signature_set[0], "count": signature_set[1], "s": s, "ent_hash": ent_hash, "ent_genome": ent_genome,
            "n_b": len(references), "cn": cn, "cd": cd}


def pool_references(n, s, seed):
    """n references out of the pool sc.random_set(.., s, ..) draws its signatures from, and of hashes outside it: empty ones,
    one hash, the whole pool, and random parts"""
    pool = sc.distinct_hashes(np.random.default_rng(s), 3 * s + 2)
    g = np.random.default_rng(seed)
    other = sc.distinct_hashes(g, 2 * s + 3)
    out = []
    for i in range(n):
        kind = (i + seed) % 5
        if kind == 0:
            out.append(np.zeros(0, np.uint32))
        elif kind == 1:
            out.append(pool[i % len(pool): i % len(pool) + 1])
        elif kind == 2:
            out.append(np.concatenate([pool, other[: s // 2]]))
        else:
            out.append(np.concatenate([g.choice(pool, size=int(g.integers(1, len(pool) + 1)), replace=False), other[: int(g.integers(0, len(other)))]]))
    return out


RUNS = (1, 63, 64, 65, 513, 600)           # the number of references the hashes of run_case() sit in; the last is all of them


def run_case():
    """s = 8, 600 references: hash 1000 + j sits in RUNS[j] references chosen at random, and every reference has a hash of its own"""
    g = np.random.default_rng(77)
    n_b = RUNS[-1]
    references = [[5000 + r] for r in range(n_b)]
    for j, n in enumerate(RUNS):
        for r in g.choice(n_b, size=n, replace=False):
            references[int(r)].append(1000 + j)
    sigs = sc.signature_set([[1000 + j for j in range(len(RUNS))] + [3, 9999], [1003, 1004], [1005], [1000, 5000 + 599], [1, 2, 3]], 8)
    return contain_case(sigs, references, 8, cn=1, cd=8)


def slice_case(n_b, slice_):
    """s = 4, references around the slice: reference r holds the hash own(r), and every third one the hash 7 as well.  Query 0
    holds own() of the references slice - 2, slice - 1 and slice (those that exist), query 1 the hash 7 -- a run through every
    slice -- with own(0) and own(n_b - 1), query 2 nothing, query 3 only hashes no reference has."""
    own = (np.arange(n_b, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(1 << 32)       # a bijection of uint32
    references = [[int(own[r])] + ([7] if r % 3 == 0 else []) for r in range(n_b)]
    near = [int(own[r]) for r in (slice_ - 2, slice_ - 1, slice_) if r < n_b]
    sigs = sc.signature_set([near, [7, int(own[0]), int(own[n_b - 1])], [], [8, 9]], 4)
    return contain_case(sigs, references, 4, cn=1, cd=4)


def boundary_case(cn, cd):
    """s = 7: reference 0 holds 3 of the query's 7 elements, reference 1 all 7, reference 2 again 3, reference 3 none"""
    sigs = sc.signature_set([[1, 2, 3, 4, 5, 6, 7]], 7)
    return contain_case(sigs, [[1, 2, 3, 8, 9], [1, 2, 3, 4, 5, 6, 7, 100], [5, 6, 7], [50, 60]], 7, cn=cn, cd=cd)


BOUNDARIES = {"met": (3000, 7000), "missed_by_one": (3001, 7000), "all": (0, 1), "only_whole": (1, 1),
              "wide_met": (3 * 306783378, 7 * 306783378), "wide_missed": (3 * 306783378 + 1, 7 * 306783378)}


@functools.lru_cache(maxsize=None)
def contain_cases():
    out = {}
    for s in SIZES:                                                   # counts of 0, 1, s - 1, s / 2 and s in every set
        out[f"pool_s{s}"] = contain_case(sc.random_set(7, s, 11 * s), pool_references(11, s, 5 * s + 1), s, cn=1, cd=8)
    out["pool_s1000_all_kept"] = contain_case(sc.random_set(7, 1000, 11000), pool_references(11, 1000, 5001), 1000)
    for s in (1, 2, 8):                                               # 0 and 0xFFFFFFFF: the two ends of the directory
        sigs = sc.signature_set([[0], [MAX_HASH], [0, MAX_HASH][:s], [5], []], s)
        out[f"extreme_hashes_s{s}"] = contain_case(sigs, [[0, MAX_HASH], [0], [MAX_HASH], [5, 6], [], [0, 5, MAX_HASH]], s)
    out["runs_s8"] = run_case()
    full = np.sort(sc.distinct_hashes(np.random.default_rng(4096), 4096))
    out["both_halves_full_s4096"] = contain_case(sc.signature_set([full, full[:2048]], 4096),
                                                 [full[::2], [], full, np.concatenate([full, [1, 2, 3]]), full[1::2]], 4096, cn=1, cd=2)
    slice_ = slice_size()
    for n_b in (slice_ - 1, slice_, slice_ + 1):
        out[f"slice_{n_b - slice_:+d}"] = slice_case(n_b, slice_)
    several = sc.random_set(5, 64, 64)
    out["no_queries_s64"] = contain_case(sc.signature_set([], 64), pool_references(4, 64, 1), 64)
    out["one_query_s64"] = contain_case((several[0][1:2], several[1][1:2]), pool_references(4, 64, 2), 64)
    out["no_entries_s64"] = contain_case(several, [[], [], []], 64)
    out["no_entries_s64_cut"] = contain_case(several, [[], [], []], 64, cn=1, cd=64)
    out["no_references_s64"] = contain_case(several, [], 64)
    # every one of 80 x 80 pairs shares the hash 42: more records than a caller's first guess at the buffer
    out["common_hash_s8"] = contain_case(sc.signature_set([[42, 1000 + i, 2000 + i] for i in range(80)], 8),
                                         [[42, 1000 + r] for r in range(80)], 8, cn=1, cd=4)
    for label, (cn, cd) in BOUNDARIES.items():
        out[f"boundary_{label}"] = boundary_case(cn, cd)
    return out
