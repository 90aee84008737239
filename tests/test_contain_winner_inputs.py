"""The cases of tests/contain_winner.py, on the CPU: the restatement of the winner-take-all statistic equals a second
definition with Python sets and dicts, every case holds what it is there for, the new symbol is what the header says, bad
parameters are refused before any device work, the family fixture has the property the end-to-end test relies on, and the
Python face validates its weights."""
import collections
import ctypes as C
import os

import numpy as np
import pytest
import torch

import contain as ct
import contain_winner as cw
import screen as sc
from conftest import ROOT, has_gpu
from pyfastani_amd import _lib, screen
from pyfastani_amd.screen import SCREEN_DTYPE
from test_contain_inputs import PIECE, fixture_minimizers

CASES = cw.winner_cases()


# ---- the second definition: Python sets and dicts ----------------------------------------------------------------------
def winner_by_dicts(case, weight):
    """(records, visited, assigned, winners) with every step spelled out: who holds a hash, how many of the query's hashes a
    reference holds, and per hash the holder that is best by (first, weight, smaller number)"""
    holders = collections.defaultdict(list)
    for h, g in zip(case["ent_hash"].tolist(), case["ent_genome"].tolist()):
        holders[h].append(g)
    weight = [0] * case["n_b"] if weight is None else [int(w) for w in weight]
    out, visited, assigned, winners = [], 0, 0, []
    for a, (row, c) in enumerate(zip(case["sig"], case["count"].tolist())):
        elements = row[:c].tolist()
        first = collections.Counter(g for x in elements for g in holders.get(x, ()))
        visited += sum(first.values())
        winner = [max(holders[x], key=lambda b: (first[b], weight[b], -b)) if x in holders else -1 for x in elements]
        won = collections.Counter(b for b in winner if b >= 0)
        assigned += sum(won.values())
        winners.append(winner)
        for b in range(case["n_b"]):
            if c and won[b] * case["cd"] >= case["cn"] * c:               # (Python integers: no overflow)
                out.append((a, b, won[b], c))
    return out, visited, assigned, winners


@pytest.mark.parametrize("name", sorted(CASES))
def test_winner_restatement_equals_the_dict_definition(name):
    case, weight = CASES[name]
    records, (evaluated, kept, visited, assigned), winners = cw.restate_winner(case, weight)
    want, want_visited, want_assigned, want_winners = winner_by_dicts(case, weight)
    assert records.dtype == SCREEN_DTYPE and [tuple(r) for r in records.tolist()] == want
    assert evaluated == len(case["count"]) * case["n_b"] and kept == len(records)
    assert visited == want_visited and assigned == want_assigned
    assert [w.tolist() for w in winners] == want_winners and all(w.dtype == np.int32 for w in winners)
    # what the header promises of the sums: first is the plain statistic, and the won of a query are its elements found anywhere
    assert visited == ct.restate_contained(case)[1][2]
    found = sum(int(np.isin(row[:c], case["ent_hash"]).sum()) for row, c in zip(case["sig"], case["count"]))
    assert assigned == found <= visited


# ---- what each case is there for -------------------------------------------------------------------------------------
def stat(records):
    return {(int(r["a"]), int(r["b"])): int(r["shared"]) for r in records}


def test_the_ties_go_to_the_weight_and_then_to_the_smaller_number():
    plain, _, winners = cw.restate_winner(*CASES["ties_s8_cn0"])
    assert [tuple(r) for r in plain.tolist()] == [(0, 0, 3, 8), (0, 1, 0, 8), (0, 2, 5, 8)]      # r1 is kept with won == 0 at cn == 0
    assert winners[0].tolist() == [2, 0, 0, 0, 2, 2, 2, 2]                                        # 2 wins 1: first 5 against 4
    assert [tuple(r) for r in cw.restate_winner(*CASES["ties_s8_cn1"])[0].tolist()] == [(0, 0, 3, 8), (0, 2, 5, 8)]
    assert cw.restate_winner(*CASES["ties_s8_cn0_zero_weights"])[0].tobytes() == plain.tobytes()
    assert stat(cw.restate_winner(*CASES["ties_s8_cn0_weight_on_1"])[0]) == {(0, 0): 0, (0, 1): 3, (0, 2): 5}
    # a weight never beats a larger first: 2 still wins the hash 1
    assert stat(cw.restate_winner(*CASES["ties_s8_cn0_weights_on_0_and_1"])[0]) == {(0, 0): 3, (0, 1): 0, (0, 2): 5}
    first = stat(ct.restate_contained(CASES["ties_s8_cn0"][0])[0])
    assert first == {(0, 0): 4, (0, 1): 4, (0, 2): 5}


def test_the_designed_winners_sit_where_the_plan_says():
    case, designed, tied = cw.positions_case()
    plan = cw.position_plan()
    assert case["n_b"] == 600 and len(plan) == len(designed) == 16 and len(tied) == len(cw.TIED)
    for length in ct.RUNS:                                             # every position that exists, and no other
        assert [p for n, p in plan if n == length] == sorted({p for p in (0, 63, 64, length - 1) if p < length})
    assert {p for _, p in plan} >= {0, 62, 63, 64, 512, 599}           # the lane walk's last entry, the wave's first, a later trip
    _, (_, _, visited, assigned), winners = cw.restate_winner(case)
    for q, (length, p) in enumerate(plan):
        run = case["ent_genome"][case["ent_hash"] == 1000 + q]
        assert len(run) == length and run[p] == designed[q] and np.all(np.diff(run) > 0)
        assert winners[q].tolist() == [designed[q]] * 3
    assert assigned == 3 * len(winners) and visited == sum(n for n, _ in plan) + sum(n for n, _, _ in cw.TIED) + 2 * (16 + 2 * 3)
    # the ties: both hold three of the query's hashes; the smaller number wins, the larger one when the weights ascend
    ascending = cw.restate_winner(*CASES["winner_positions_s8_ascending_weights"])[2]
    for i, ((length, pa, pb), (ra, rb)) in enumerate(zip(cw.TIED, tied)):
        q = len(plan) + i
        run = case["ent_genome"][case["ent_hash"] == 1000 + q]
        assert len(run) == length and (run[pa], run[pb]) == (ra, rb) and ra < rb
        assert winners[q].tolist() == [ra] * 3 and ascending[q].tolist() == [rb] * 3
    assert cw.TIED[0][1] >= 64 and cw.TIED[1][1] < 64 <= cw.TIED[1][2]      # both by the wave; one by the lane and one by the wave
    assert set(CASES["winner_positions_s8_weighted"][1].tolist()) == {0, 1, 2, 3}           # 600 weights of four values: they tie


def test_the_cross_slice_cases_carry_a_hash_across_the_slices():
    slice_ = ct.slice_size()
    assert sorted(cw.cross_slice_sizes().values()) == [slice_ - 1, slice_, slice_ + 1, 2 * slice_ + 1]
    for label, n_b in cw.cross_slice_sizes().items():
        last, t = n_b - 1, cw.last_third(n_b)
        case = CASES[f"cross_slice_{label}_none"][0]
        run = case["ent_genome"][case["ent_hash"] == 7]
        assert case["n_b"] == n_b and run[0] == 0 and run[-1] == last and run[-2] == t and t % 3 == 0 and 3 < t < last
        # the slices of the run's head, of t and of the last reference: the winners of queries 0 .. 2 lie behind the head
        assert (0, t // slice_, last // slice_) == {"slice-1": (0, 0, 0), "slice": (0, 0, 0), "slice+1": (0, 0, 1), "2slice+1": (0, 1, 2)}[label]
        want = {"none": (0, 3), "on_t": (0, t), "on_last": (last, t)}
        for name, (q1, q2) in want.items():
            records, (evaluated, kept, visited, assigned), winners = cw.restate_winner(*CASES[f"cross_slice_{label}_{name}"])
            assert winners[0].tolist().count(last) == 2 and winners[1].tolist().count(q1) == 2 and winners[2].tolist().count(q2) == 2
            assert len(winners[3]) == 0 and winners[4].tolist() == [-1, -1]
            assert evaluated == 5 * n_b and assigned == 2 + 3 + 3 and visited == 3 * len(run) + 1 + 2 + 2
            # who loses the tie keeps its own hash: won == 1 of 3, kept at cn / cd == 1 / 4
            assert stat(records)[0, last] == 2 and sorted(v for (a, _), v in stat(records).items() if a == 1) == [1, 2]
            assert kept == 1 + 2 + 2


def test_every_plain_case_runs_under_the_winner_rule_with_and_without_weights():
    for name, case in ct.contain_cases().items():
        assert CASES[name][0] is case and CASES[name][1] is None and CASES[name + "_weighted"][0] is case
        weight = CASES[name + "_weighted"][1]
        assert weight.dtype == np.int32 and weight.shape == (case["n_b"],) and (len(weight) < 8 or len(set(weight.tolist())) < len(weight))
    records, (_, _, visited, assigned), _ = cw.restate_winner(*CASES["both_halves_full_s4096"])
    assert records["shared"].max() == 4096 and assigned == 4096 + 2048 and visited == 12288 + 6144


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_symbol():
    header = open(os.path.join(ROOT, "include", "fastani_hip.h")).read()
    assert "int fa_screen_contained_winner(" in header and "const int32_t *d_weight" in header
    assert "fa_screen_contained_winner" in _lib.SIGNATURES and hasattr(_lib.lib, "fa_screen_contained_winner")
    plain, winner = _lib.SIGNATURES["fa_screen_contained"][1], _lib.SIGNATURES["fa_screen_contained_winner"][1]
    assert len(winner) == len(plain) + 1 and winner[:8] == plain[:8] and winner[9:] == plain[8:]      # d_weight behind n_b


def call(n_a=0, s=8, n_entries=0, n_b=0, weight=None, cn=0, cd=1, pairs=None, cap=0, sig=None, ent=None):
    n = C.c_int64(-1)
    code = _lib.lib.fa_screen_contained_winner(sig, sig, n_a, s, ent, ent, n_entries, n_b, weight, cn, cd, pairs, cap, C.byref(n), 0, None)
    return code, n.value


def test_bad_parameters_are_reported_before_any_device_work():
    error = _lib.lib.fa_last_error
    for s in (0, -3, 4097):
        assert call(s=s) == (_lib.FA_ERR_INVALID, -1) and b"[1, 4096]" in error()
    for cn, cd in ((-1, 4), (5, 4), (0, 0), (1, -1)):
        assert call(cn=cn, cd=cd) == (_lib.FA_ERR_INVALID, -1) and b"cn <= cd" in error()
    assert call(n_a=3) == (_lib.FA_ERR_INVALID, -1) and b"null signatures" in error()
    assert call(n_entries=3, n_b=2) == (_lib.FA_ERR_INVALID, -1) and b"null entries" in error()
    assert call(n_b=-2) == (_lib.FA_ERR_INVALID, -1)
    assert call(n_a=-1) == (_lib.FA_ERR_INVALID, -1)
    assert call(n_entries=-1) == (_lib.FA_ERR_INVALID, -1)
    assert call(n_b=2, pairs=C.c_void_p(8), cap=-1) == (_lib.FA_ERR_INVALID, -1) and b"negative capacity" in error()
    assert _lib.lib.fa_debug_contain_winner_threads(256) == _lib.FA_ERR_INVALID
    assert _lib.lib.fa_debug_contain_winner_threads(0) == _lib.FA_OK


@pytest.mark.skipif(has_gpu(), reason="CPU-only behaviour")
def test_without_a_device_the_winner_road_fails_loudly():
    assert call() == (_lib.FA_ERR_NO_DEVICE, -1)
    assert b"no HIP device" in _lib.lib.fa_last_error()
    assert call(n_b=3, weight=C.c_void_p(8)) == (_lib.FA_ERR_NO_DEVICE, -1)


# ---- the end-to-end fixture ------------------------------------------------------------------------------------------
def test_the_source_of_a_piece_holds_more_of_it_than_any_other_genome():
    """what the GPU test expects of winner_take_all end to end is a property of the genomes: member 1 of a family holds every
    hash of the piece cut from it and every other genome strictly fewer, so it wins them all without a tie"""
    h, seq = fixture_minimizers()
    assert PIECE == slice(20_000, 25_000)
    sig, count = sc.restate_signatures({"hash": h, "seq_id": seq, "sbf": np.arange(1, 16, dtype=np.int32), "s": 1000})
    refs = seq < 12
    ent_hash, ent_genome = ct.restate_contents({"hash": h[refs], "seq_id": seq[refs], "sbf": np.arange(1, 13, dtype=np.int32)})
    case = {"sig": sig[12:], "count": count[12:], "s": 1000, "ent_hash": ent_hash, "ent_genome": ent_genome, "n_b": 12, "cn": 0, "cd": 1}
    first = stat(ct.restate_contained(case)[0])
    for p in range(sc.FAMILIES):
        denom = int(count[12 + p])
        assert first[p, 4 * p + 1] == denom
        assert all(first[p, b] < denom for b in range(12) if b != 4 * p + 1)
    records, (evaluated, kept, visited, assigned), winners = cw.restate_winner(case)
    cut = records[screen.identity(records, 16) >= 0.88]
    assert [tuple(r) for r in cut.tolist()] == [(p, 4 * p + 1, int(count[12 + p]), int(count[12 + p])) for p in range(3)]
    assert assigned == int(count[12:].sum()) and all(np.all(w == 4 * p + 1) for p, w in enumerate(winners))


# ---- the Python face -------------------------------------------------------------------------------------------------
def host_contents(n, lengths=None):
    empty = torch.zeros(0, dtype=torch.int32)
    return screen.Contents(empty, empty, [f"r{i}" for i in range(n)], 16, lengths)


def test_contents_keep_their_lengths():
    assert host_contents(3).lengths is None
    kept = host_contents(3, np.array([5, 2 ** 40, 0], dtype=np.uint64)).lengths
    assert kept.dtype == np.int64 and kept.tolist() == [5, 2 ** 40, 0]
    assert host_contents(2, [7, 8]).lengths.tolist() == [7, 8]
    with pytest.raises(ValueError, match="one length per genome"):
        host_contents(3, [1, 2])


def test_weights_are_validated_before_any_device_work():
    sigs = screen.Signatures(torch.zeros((1, 8), dtype=torch.int32), torch.zeros(1, dtype=torch.int32), ["q"], 16)
    contents = host_contents(3, [10, 2 ** 40, 30])
    for bad in ([1, 2], [1, 2, 3, 4], np.array([1, -1, 0]), torch.tensor([0, 0, -5]), [0.5, 1.0, 2.0], [0, 2 ** 31, 0], "size"):
        with pytest.raises(ValueError):
            screen.contained(sigs, contents, winner_take_all=True, weights=bad)
    for weights in ([1, 2, 3], "length", None):
        if weights is not None:
            with pytest.raises(ValueError, match="winner_take_all"):
                screen.contained(sigs, contents, weights=weights)
    with pytest.raises(ValueError, match="lengths"):
        screen.contained(sigs, host_contents(3), winner_take_all=True, weights="length")
    assert screen._winner_weights("length", contents).tolist() == [10, 2 ** 31 - 1, 30]      # clipped to int32
    for good in ([1, 2, 3], (0, 0, 0), np.array([3, 2, 1], dtype=np.int64), torch.tensor([4, 5, 6])):
        got = screen._winner_weights(good, contents)
        assert got.dtype == np.int32 and got.flags["C_CONTIGUOUS"] and got.tolist() == [int(v) for v in good]
