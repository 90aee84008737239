"""Winner-take-all containment on the device (fa_screen_contained_winner, screen.contained(.., winner_take_all=True)) against
the plain restatement of tests/contain_winner.py -- MI355X only.  Records are compared byte for byte, *n_pairs and the four
counters exactly.  The inputs are synthetic signatures and directories but for the last test, which sketches genomes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import contain as ct
import contain_winner as cw
import screen as sc
from pyfastani_amd import _lib, outputs, screen
from pyfastani_amd._lib import FA_ERR_INVALID, FA_OK, lib
from pyfastani_amd.screen import SCREEN_DTYPE

pytestmark = pytest.mark.gpu

CASES = cw.winner_cases()
DEVICE = "cuda:0"
RECORDS = 40000                             # no case keeps more


def to_device(array):
    """the bytes of a numpy array in HBM (uint32 has no torch dtype everywhere: the words travel as int32)"""
    flat = np.ascontiguousarray(array).reshape(-1)
    return torch.from_numpy(flat.view(np.int32).copy()).to(DEVICE)


def ptr(tensor):
    return C.c_void_p(tensor.data_ptr()) if tensor is not None and tensor.numel() else None


@functools.lru_cache(maxsize=None)
def expected(name):
    return cw.restate_winner(*CASES[name])[:2]


def lib_winner(case, weight=None, pairs_device=False, cap=None, count_only=False, changes=None, **replaced):
    """(status, the whole record buffer as bytes, *n_pairs, stats); the buffer starts as bytes 0xAB, *n_pairs as -1 and stats
    as -1s.  ``changes(sig, count, ent_hash, ent_genome)`` edits copies of the inputs; ``replaced`` replace s, cn, cd, n_b."""
    arrays = [case[key].copy() for key in ("sig", "count", "ent_hash", "ent_genome")]
    if changes:
        changes(*arrays)
    d_sig, d_count, d_ent_hash, d_ent_genome = (to_device(a) for a in arrays)
    d_weight = None if weight is None else to_device(np.asarray(weight, dtype=np.int32))
    n_a, n_b = len(case["count"]), replaced.get("n_b", case["n_b"])
    cap = min(n_a * n_b, RECORDS) + 3 if cap is None else cap
    n, stats = C.c_int64(-1), (C.c_int64 * 4)(-1, -1, -1, -1)
    head = (ptr(d_sig), ptr(d_count), n_a, replaced.get("s", case["s"]), ptr(d_ent_hash), ptr(d_ent_genome), len(case["ent_hash"]), n_b,
            ptr(d_weight), replaced.get("cn", case["cn"]), replaced.get("cd", case["cd"]))
    buffer = np.full(cap * 16, 0xAB, dtype=np.uint8)
    torch.cuda.synchronize()
    if pairs_device:
        d_buffer = torch.from_numpy(buffer.copy()).to(DEVICE)
        torch.cuda.synchronize()
        code = lib.fa_screen_contained_winner(*head, None if count_only else C.c_void_p(d_buffer.data_ptr()), cap, C.byref(n), 1, stats)
        buffer = d_buffer.cpu().numpy()
    else:
        code = lib.fa_screen_contained_winner(*head, None if count_only else C.c_void_p(buffer.ctypes.data), cap, C.byref(n), 0, stats)
    return code, buffer, n.value, tuple(stats)


def check(name, got, count_only=False):
    code, buffer, n, stats = got
    want, want_stats = expected(name)
    assert code == FA_OK, _lib.last_error()
    assert n == len(want) and stats == want_stats, (n, len(want), stats, want_stats)
    written = 0 if count_only else n * 16
    assert buffer[:written].tobytes() == want.tobytes()[:written]
    assert np.all(buffer[written:] == 0xAB)                                 # nothing is written behind the records


def untouched(got):
    return np.all(got[1] == 0xAB) and got[3] == (-1, -1, -1, -1)


# ---- every case, through the C ABI -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_records_and_counters_match_the_restatement(name):
    case, weight = CASES[name]
    assert len(expected(name)[0]) <= RECORDS
    check(name, lib_winner(case, weight))
    check(name, lib_winner(case, weight, count_only=True), count_only=True)


def test_the_ties():
    """the figures of the issue's example, read off the device's records"""
    def won(name):
        code, buffer, n, stats = lib_winner(*CASES[name])
        assert code == FA_OK
        return [tuple(r) for r in buffer[: n * 16].view(SCREEN_DTYPE).tolist()], stats
    assert won("ties_s8_cn0") == ([(0, 0, 3, 8), (0, 1, 0, 8), (0, 2, 5, 8)], (3, 3, 13, 8))
    assert won("ties_s8_cn1") == ([(0, 0, 3, 8), (0, 2, 5, 8)], (3, 2, 13, 8))
    assert won("ties_s8_cn0_weight_on_1")[0] == [(0, 0, 0, 8), (0, 1, 3, 8), (0, 2, 5, 8)]
    assert won("ties_s8_cn0_weights_on_0_and_1")[0] == [(0, 0, 3, 8), (0, 1, 0, 8), (0, 2, 5, 8)]
    assert won("ties_s8_cn0_zero_weights") == won("ties_s8_cn0")


def test_the_thread_count_does_not_change_a_byte():
    try:
        for threads in (1024, 512):
            assert lib.fa_debug_contain_winner_threads(threads) == FA_OK
            for name in ("winner_positions_s8_weighted", "both_halves_full_s4096_weighted", "pool_s1000", "cross_slice_2slice+1_on_last"):
                check(name, lib_winner(*CASES[name]))
    finally:
        assert lib.fa_debug_contain_winner_threads(0) == FA_OK


# ---- plumbing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pool_s1000_weighted", "winner_positions_s8", "cross_slice_slice+1_on_t", "both_halves_full_s4096",
                                  "no_references_s64"])
def test_host_and_device_records_agree(name):
    check(name, lib_winner(*CASES[name], pairs_device=True))
    check(name, lib_winner(*CASES[name], pairs_device=False))


@pytest.mark.parametrize("pairs_device", [False, True])
def test_a_buffer_one_record_short_is_invalid(pairs_device):
    name = "runs_s8_weighted"
    n_records = len(expected(name)[0])
    assert n_records > 4
    got = lib_winner(*CASES[name], pairs_device=pairs_device, cap=n_records - 1)
    assert got[0] == FA_ERR_INVALID and untouched(got), _lib.last_error()
    assert got[2] == n_records                                              # what the caller needs
    check(name, lib_winner(*CASES[name], pairs_device=pairs_device, cap=n_records))


def test_the_same_input_gives_the_same_bytes():
    for name in ("pool_s1000_weighted", "winner_positions_s8_weighted", "cross_slice_2slice+1_on_t"):
        runs = [lib_winner(*CASES[name], pairs_device=True) for _ in range(3)]
        for run in runs:
            check(name, run)
            assert run[1].tobytes() == runs[0][1].tobytes()


def bad_inputs():
    from test_gpu_contain import BAD_INPUTS
    return BAD_INPUTS


@pytest.mark.parametrize("label", sorted(bad_inputs()))
def test_bad_inputs_are_invalid_and_return_nothing(label):
    name = "pool_s1000_weighted"
    case, weight = CASES[name]
    assert case["count"][[0, 3, 6]].tolist() == [1000, 1000, 1000] and case["n_b"] == 11
    for pairs_device in (False, True):
        got = lib_winner(case, weight, pairs_device=pairs_device, changes=bad_inputs()[label])
        assert got[0] == FA_ERR_INVALID and got[2] == -1 and untouched(got), (got[0], got[2], got[3], _lib.last_error())
    check(name, lib_winner(case, weight))                                   # the process goes on


@pytest.mark.parametrize("at", [0, 5, 10])
def test_a_negative_weight_is_invalid_and_returns_nothing(at):
    name = "pool_s1000_weighted"
    case, weight = CASES[name]
    bad = weight.copy()
    bad[at] = -1 if at else -2 ** 31
    for pairs_device in (False, True):
        got = lib_winner(case, bad, pairs_device=pairs_device)
        assert got[0] == FA_ERR_INVALID and got[2] == -1 and untouched(got) and "weight" in _lib.last_error()
    # also where there is nothing else to check: no query, no entry
    nothing = dict(case, sig=case["sig"][:0], count=case["count"][:0], ent_hash=case["ent_hash"][:0], ent_genome=case["ent_genome"][:0])
    got = lib_winner(nothing, bad)
    assert got[0] == FA_ERR_INVALID and got[2] == -1 and untouched(got)
    check(name, lib_winner(case, weight))


def test_bad_parameters_return_nothing():
    case, weight = CASES["pool_s64_weighted"]
    for replaced in (dict(s=0), dict(s=4097), dict(cn=-1), dict(cn=2, cd=1), dict(cd=0), dict(n_b=10), dict(n_b=-1)):
        got = lib_winner(case, None if "n_b" in replaced else weight, cap=80, **replaced)
        assert got[0] == FA_ERR_INVALID and got[2] == -1 and untouched(got), replaced


# ---- the Python face ---------------------------------------------------------------------------------------------------
def as_signatures(case, k=16):
    n = len(case["count"])
    return screen.Signatures(to_device(case["sig"]).view(n, -1), to_device(case["count"]), [f"q{i}" for i in range(n)], k)


def as_contents(case, k=16, lengths=None):
    return screen.Contents(to_device(case["ent_hash"]), to_device(case["ent_genome"]), [f"r{i}" for i in range(case["n_b"])], k, lengths)


@pytest.mark.parametrize("name", ["pool_s1000", "pool_s1000_weighted"])
def test_python_winner_take_all_cut_by_identity(name):
    case, weight = CASES[name]
    sigs, contents = as_signatures(case), as_contents(case, lengths=weight)
    everything, (evaluated, _, visited, assigned), _ = cw.restate_winner(dict(case, cn=0, cd=1), weight)
    sizes = []
    for cut in (0.0, 0.9, 1.0):
        want = everything[screen.identity(everything, 16) >= cut]
        for weights in ([None] if weight is None else [weight, weight.tolist(), torch.from_numpy(weight), "length"]):
            stats = {}
            got = screen.contained(sigs, contents, min_identity=cut, stats=stats, winner_take_all=True, weights=weights)
            assert got.dtype == SCREEN_DTYPE and got.tobytes() == want.tobytes()
            assert stats["evaluated"] == evaluated == 77 and stats["visited"] == visited and stats["assigned"] == assigned > 0
            assert len(want) <= stats["kept"] <= len(everything)
        on_device = screen.contained(sigs, contents, min_identity=cut, device=True, winner_take_all=True, weights=weight)
        assert on_device.is_cuda and on_device.dtype == torch.int32 and screen.to_records(on_device).tobytes() == want.tobytes()
        sizes.append(len(want))
    assert sizes[0] == len(everything) > sizes[1] >= sizes[2] > 0


def test_python_without_the_flag_is_the_plain_road():
    case = CASES["pool_s1000"][0]
    sigs, contents = as_signatures(case), as_contents(case)
    everything, (evaluated, _, visited) = ct.restate_contained(dict(case, cn=0, cd=1))
    want = everything[screen.identity(everything, 16) >= 0.9]
    stats = {}
    got = screen.contained(sigs, contents, min_identity=0.9, stats=stats)
    assert got.tobytes() == want.tobytes() and len(want) > 0
    assert "assigned" not in stats and stats["visited"] == visited and stats["evaluated"] == evaluated
    both = screen.contained(sigs, contents, min_identity=0.9, winner_take_all=True)
    assert both.tobytes() != got.tobytes()                                  # the two statistics differ on this case


def test_python_sizing_retry():
    """every one of 80 x 80 pairs shares the hash 42 and the device filter is off: 6400 records, more than the first buffer holds"""
    wide = CASES["common_hash_s8"][0]
    want, (_, kept, _, assigned), _ = cw.restate_winner(dict(wide, cn=0, cd=1))
    stats = {}
    got = screen.contained(as_signatures(wide), as_contents(wide), min_identity=0.0, winner_take_all=True, stats=stats)
    assert kept == 6400 > max(4096, 16 * 160) and got.tobytes() == want.tobytes()
    assert stats["kept"] == 6400 and stats["assigned"] == assigned == 80 * 2


def test_pieces_end_to_end(tmp_path):
    """The fixture of test_gpu_contain.test_pieces_end_to_end: a 5 kb piece of member 1 of each of three families finds members
    0, 1 and 2 of its family by plain containment, nine records -- and under winner_take_all its source alone, three records
    that hold every hash of the piece (tests/test_contain_winner_inputs.py has the property of the genomes behind this)."""
    import pyfastani_amd as pf
    genomes = sc.family_genomes()
    pieces = [genomes[4 * f + 1][20_000:25_000] for f in range(sc.FAMILIES)]
    references, queries = pf.Sketch(), pf.Sketch()
    for i, genome in enumerate(genomes):
        references.add_genome(f"genome{i}", genome)
    for f, piece in enumerate(pieces):
        queries.add_genome(f"piece{f}", piece)
    contents = screen.contents(references)
    whole = references.fragment_length                                       # the sketch counts a contig in whole fragments
    assert contents.lengths.dtype == np.int64 and contents.lengths.tolist() == [len(g) // whole * whole for g in genomes] == [99_000] * 12
    sigs = screen.signatures(queries, size=1000)
    plain = screen.contained(sigs, contents, min_identity=0.88)
    assert [(int(r["a"]), int(r["b"])) for r in plain] == [(p, 4 * p + m) for p in range(3) for m in (0, 1, 2)]          # the nine records
    stats = {}
    records = screen.contained(sigs, contents, min_identity=0.88, winner_take_all=True, stats=stats)
    assert [(int(r["a"]), int(r["b"])) for r in records] == [(p, 4 * p + 1) for p in range(3)]                           # the three
    assert np.all(records["shared"] == records["denom"]) and records["denom"].tolist() == sigs.count.cpu().numpy().tolist()
    assert stats["evaluated"] == 36 and stats["assigned"] == int(records["denom"].sum()) and stats["visited"] > stats["assigned"]
    case = {"sig": sigs.sig.cpu().numpy().view(np.uint32), "count": sigs.count.cpu().numpy(), "s": 1000,
            "ent_hash": contents.hash.cpu().numpy().view(np.uint32), "ent_genome": contents.genome.cpu().numpy(), "n_b": 12, "cn": 0, "cd": 1}
    want, _, _ = cw.restate_winner(case)
    assert records.tobytes() == want[screen.identity(want, 16) >= 0.88].tobytes()
    by_length = screen.contained(sigs, contents, min_identity=0.88, winner_take_all=True, weights="length")
    assert by_length.tobytes() == records.tobytes()                         # there is no tie for a weight to break
    outputs.write_containment(tmp_path / "winner.tsv", sigs.names, contents.names, records, sigs.k)
    lines = (tmp_path / "winner.tsv").read_text().splitlines()
    assert len(lines) == 3 and all(line.startswith(f"piece{p}\tgenome{4 * p + 1}\t1\t") for p, line in enumerate(lines))
