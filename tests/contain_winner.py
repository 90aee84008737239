"""The winner-take-all statistic of the containment road (fa_screen_contained_winner, pyfastani_amd/csrc/fa_contain.hip.h),
restated in plain numpy, and the named cases both of its test files run next to those of tests/contain.py.

  first     np.bincount of the genomes of the directory's entries whose hash is in the signature
  winner    those entries sorted by (hash, first descending, weight descending, genome): the first of every hash
  won       np.bincount of the winners; the filter of tests/contain.py on won, in int64
  visited   the sum of first;  assigned   the sum of won

tests/test_contain_winner_inputs.py checks the restatement on the CPU against a second definition with Python sets and dicts;
tests/test_gpu_contain_winner.py compares the library with it byte for byte.
"""
import functools

import numpy as np

import contain as ct
import screen as sc
from pyfastani_amd.screen import SCREEN_DTYPE


# ---- the restatement -------------------------------------------------------------------------------------------------
def restate_winner(case, weight=None):
    """(records SCREEN_DTYPE sorted by (a, b), (evaluated, kept, visited, assigned), the winners: per query an int32 array,
    one per element of the signature, -1 for an element no reference holds)"""
    n_a, n_b, out, visited, assigned, winners = len(case["count"]), case["n_b"], [], 0, 0, []
    weight = np.zeros(n_b, dtype=np.int64) if weight is None else np.asarray(weight, dtype=np.int64)
    assert weight.shape == (n_b,)
    for a in range(n_a):
        mine = case["sig"][a, : case["count"][a]]
        denom = len(mine)
        hit = np.isin(case["ent_hash"], mine)
        h, g = case["ent_hash"][hit], case["ent_genome"][hit].astype(np.int64)
        first = np.bincount(g, minlength=n_b)
        order = np.lexsort((g, -weight[g], -first[g], h))             # (the last key is the first to sort by)
        h, g = h[order], g[order]
        head = np.ones(len(h), dtype=bool)
        head[1:] = h[1:] != h[:-1]
        winner = np.full(denom, -1, dtype=np.int32)
        winner[np.searchsorted(mine, h[head])] = g[head]
        won = np.bincount(g[head], minlength=n_b)
        visited += int(first.sum())
        assigned += int(won.sum())
        winners.append(winner)
        if denom:                                                     # (won <= 4096 and cn, cd < 2^31: the products are below 2^63)
            kept = np.nonzero(won.astype(np.int64) * int(case["cd"]) >= int(case["cn"]) * denom)[0]
            out += [(a, int(b), int(won[b]), denom) for b in kept]
    return np.array(out, dtype=SCREEN_DTYPE), (n_a * n_b, len(out), visited, assigned), winners


# ---- cases -----------------------------------------------------------------------------------------------------------
def ties_case(cn=0):
    """s = 8, the query {1 .. 8}: references 0 and 1 hold {1, 2, 3, 4} both, reference 2 {1, 5, 6, 7, 8}"""
    return ct.contain_case(sc.signature_set([[1, 2, 3, 4, 5, 6, 7, 8]], 8), [[1, 2, 3, 4], [1, 2, 3, 4], [1, 5, 6, 7, 8]], 8, cn=cn, cd=8)


POSITIONS = (0, 63, 64, -1)                 # of the designed winner in its run, -1: the last
# (run length, position a, position b): two holders of the run tie on `first`
TIED = ((600, 100, 300), (600, 10, 200), (65, 3, 64))


def position_plan():
    """[(run length, position of the designed winner)], one query each: every length of ct.RUNS with every position that exists"""
    plan = []
    for length in ct.RUNS:
        plan += [(length, p) for p in sorted({length - 1 if p < 0 else p for p in POSITIONS}) if p < length]
    return plan


def positions_case():
    """s = 8, 600 references.  Query q of position_plan() holds the hash 1000 + q, which sits in `length` references drawn at
    random, and two hashes more that only the reference at position p of that run (by genome number) holds: it has first == 3
    against 1 and wins the three.  The queries behind them, one per entry of TIED, have two such references, at positions a
    and b of the run: a tie on `first` that the smaller number wins unless the weights say otherwise.
    Returns (case, [the designed winner of query q], [(reference at a, reference at b) of the tied queries])."""
    g = np.random.default_rng(78)
    n_b = ct.RUNS[-1]
    references = [[5000 + r] for r in range(n_b)]
    queries, designed, tied = [], [], []
    for q, (length, *at) in enumerate(position_plan() + list(TIED)):
        holders = np.sort(g.choice(n_b, size=length, replace=False))
        extra = [100_000 + 2 * q, 100_001 + 2 * q]
        for r in holders:
            references[int(r)].append(1000 + q)
        for p in at:
            references[int(holders[p])] += extra
        queries.append([1000 + q] + extra)
        if len(at) == 1:
            designed.append(int(holders[at[0]]))
        else:
            tied.append((int(holders[at[0]]), int(holders[at[1]])))
    return ct.contain_case(sc.signature_set(queries, 8), references, 8, cn=1, cd=8), designed, tied


def cross_slice_case(n_b):
    """s = 4: reference r holds the hash own(r), and every third one and the last one the hash 7 as well -- a run through
    every slice.  t is the last reference before the last one that holds 7.
      query 0   {7, own(n_b - 1)}: the last reference has first == 2 and takes 7 out of every earlier slice
      query 1   {7, own(0), own(n_b - 1)}: references 0 and n_b - 1 tie on first; without a weight between them 0 keeps 7
      query 2   {7, own(3), own(t)}: the same tie between 3 and t -- cross_slice_weights() puts the weight on t
      query 3   empty;  query 4   hashes nobody has"""
    own = (np.arange(n_b, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(1 << 32)       # a bijection of uint32
    t = last_third(n_b)
    references = [[int(own[r])] + ([7] if r % 3 == 0 or r == n_b - 1 else []) for r in range(n_b)]
    sigs = sc.signature_set([[7, int(own[n_b - 1])], [7, int(own[0]), int(own[n_b - 1])], [7, int(own[3]), int(own[t])], [], [8, 9]], 4)
    return ct.contain_case(sigs, references, 4, cn=1, cd=4)


def last_third(n_b):
    return (n_b - 2) // 3 * 3


def cross_slice_weights(n_b):
    """name -> weights: none; 5 on t alone (query 2 goes to t, query 1 stays with 0); 7 on the last reference as well (query 1
    goes to it)"""
    on_t = np.zeros(n_b, dtype=np.int32)
    on_t[last_third(n_b)] = 5
    on_last = on_t.copy()
    on_last[n_b - 1] = 7
    return {"none": None, "on_t": on_t, "on_last": on_last}


def cross_slice_sizes():
    slice_ = ct.slice_size()
    return {"slice-1": slice_ - 1, "slice": slice_, "slice+1": slice_ + 1, "2slice+1": 2 * slice_ + 1}


@functools.lru_cache(maxsize=None)
def winner_cases():
    """name -> (case, weights or None): every case of ct.contain_cases() without weights and with random ones in [0, 4), so
    that weights tie too, and the cases of this file"""
    out = {}
    for name, case in ct.contain_cases().items():
        out[name] = (case, None)
        out[name + "_weighted"] = (case, np.random.default_rng(1).integers(0, 4, case["n_b"]).astype(np.int32))
    for cn in (0, 1):
        for label, weight in (("", None), ("_zero_weights", [0, 0, 0]), ("_weight_on_1", [0, 5, 0]), ("_weights_on_0_and_1", [9, 9, 0])):
            out[f"ties_s8_cn{cn}{label}"] = (ties_case(cn), None if weight is None else np.array(weight, dtype=np.int32))
    positions = positions_case()[0]
    out["winner_positions_s8"] = (positions, None)
    out["winner_positions_s8_weighted"] = (positions, np.random.default_rng(1).integers(0, 4, positions["n_b"]).astype(np.int32))
    out["winner_positions_s8_ascending_weights"] = (positions, np.arange(1, positions["n_b"] + 1, dtype=np.int32))      # ties: the larger number
    for label, n_b in cross_slice_sizes().items():
        case = cross_slice_case(n_b)
        for name, weight in cross_slice_weights(n_b).items():
            out[f"cross_slice_{label}_{name}"] = (case, weight)
    return out
