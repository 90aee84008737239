"""The containment road of the screen on the device (fa_screen_contents / fa_screen_contained, pyfastani_amd.screen) against
the plain restatement of tests/contain.py -- MI355X only.  Entries and records are compared byte for byte, the counters
exactly.  The inputs are synthetic records, signatures and directories but for the last test, which sketches genomes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import contain as ct
import screen as sc
from pyfastani_amd import _lib, outputs, screen
from pyfastani_amd._lib import FA_ERR_INVALID, FA_OK, lib
from pyfastani_amd.screen import SCREEN_DTYPE

pytestmark = pytest.mark.gpu

SIGNATURE_CASES = sc.signature_cases()
CASES = ct.contain_cases()
DEVICE = "cuda:0"


def to_device(array):
    """the bytes of a numpy array in HBM (uint32 has no torch dtype everywhere: the words travel as int32)"""
    flat = np.ascontiguousarray(array).reshape(-1)
    words = flat.view(np.int32) if flat.dtype.itemsize == 4 else flat.view(np.uint8)
    return torch.from_numpy(words.copy()).to(DEVICE)


def ptr(tensor):
    return C.c_void_p(tensor.data_ptr()) if tensor.numel() else None


# ---- contents --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_contents(name):
    return ct.restate_contents(SIGNATURE_CASES[name])


def lib_contents(case, cap=None, count_only=False):
    """(status, ent_hash bytes, ent_genome bytes, *n_entries): the outputs start as bytes 0xAB, *n_entries as -1"""
    cap = len(case["hash"]) + 3 if cap is None else cap
    d_hash, d_seq = to_device(case["hash"]), to_device(case["seq_id"])
    d_ent_hash = torch.full((max(cap, 1) * 4,), 0xAB, dtype=torch.uint8, device=DEVICE)
    d_ent_genome = torch.full((max(cap, 1) * 4,), 0xAB, dtype=torch.uint8, device=DEVICE)
    n = C.c_int64(-1)
    torch.cuda.synchronize()
    code = lib.fa_screen_contents(ptr(d_hash), ptr(d_seq), len(case["hash"]), C.c_void_p(case["sbf"].ctypes.data), len(case["sbf"]),
                                  None if count_only else C.c_void_p(d_ent_hash.data_ptr()),
                                  None if count_only else C.c_void_p(d_ent_genome.data_ptr()), cap, C.byref(n))
    return code, d_ent_hash.cpu().numpy(), d_ent_genome.cpu().numpy(), n.value


@pytest.mark.parametrize("name", sorted(SIGNATURE_CASES))
def test_contents_match_the_restatement(name):
    """with room to spare, with exactly the room needed, counting only, and one entry short"""
    case = SIGNATURE_CASES[name]
    want_hash, want_genome = expected_contents(name)
    m = len(want_hash)
    for cap in (None, m):
        code, ent_hash, ent_genome, n = lib_contents(case, cap=cap)
        assert code == FA_OK, _lib.last_error()
        assert n == m and ent_hash[: 4 * m].tobytes() == want_hash.tobytes() and ent_genome[: 4 * m].tobytes() == want_genome.tobytes()
        assert np.all(ent_hash[4 * m:] == 0xAB) and np.all(ent_genome[4 * m:] == 0xAB)      # nothing is written behind the entries
    code, ent_hash, ent_genome, n = lib_contents(case, count_only=True)
    assert code == FA_OK and n == m and np.all(ent_hash == 0xAB) and np.all(ent_genome == 0xAB)
    if m:
        code, ent_hash, ent_genome, n = lib_contents(case, cap=m - 1)
        assert code == FA_ERR_INVALID and n == m and np.all(ent_hash == 0xAB) and np.all(ent_genome == 0xAB), _lib.last_error()


def bad_records():
    case = SIGNATURE_CASES["mixed_s64"]
    out = {}
    descending = dict(case, seq_id=case["seq_id"].copy())
    descending["seq_id"][[200, 201]] = descending["seq_id"][[201, 200]] + np.array([1, 0], dtype=np.int32)
    out["contig_ids_descend"] = descending
    for label, value in (("contig_id_is_the_number_of_contigs", int(case["sbf"][-1])), ("contig_id_is_huge", 2 ** 31 - 1)):
        bad = dict(case, seq_id=case["seq_id"].copy())
        bad["seq_id"][-1] = value
        out[label] = bad
    negative = dict(case, seq_id=case["seq_id"].copy())
    negative["seq_id"][0] = -1
    out["contig_id_is_negative"] = negative
    down = dict(case, sbf=case["sbf"].copy())
    down["sbf"][3] = down["sbf"][2] - 1
    out["sbf_decreases"] = down
    return out


@pytest.mark.parametrize("label", sorted(bad_records()))
def test_bad_records_are_invalid_and_leave_the_outputs_untouched(label):
    case = bad_records()[label]
    assert label != "contig_ids_descend" or np.any(np.diff(case["seq_id"]) < 0)
    code, ent_hash, ent_genome, n = lib_contents(case)
    assert code == FA_ERR_INVALID and n == -1, (code, n, _lib.last_error())
    assert np.all(ent_hash == 0xAB) and np.all(ent_genome == 0xAB)
    test_contents_match_the_restatement("mixed_s64")                        # the process goes on


# ---- containment -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(name):
    return ct.restate_contained(CASES[name])


def lib_contained(case, pairs_device=False, cap=None, count_only=False, changes=None, **replaced):
    """(status, the whole record buffer as bytes, *n_pairs, stats); the buffer starts as bytes 0xAB, *n_pairs as -1 and stats
    as -1s.  ``changes(sig, count, ent_hash, ent_genome)`` edits copies of the inputs; ``replaced`` replace s, cn, cd, n_b."""
    arrays = [case[key].copy() for key in ("sig", "count", "ent_hash", "ent_genome")]
    if changes:
        changes(*arrays)
    d_sig, d_count, d_ent_hash, d_ent_genome = (to_device(a) for a in arrays)
    n_a, n_b = len(case["count"]), replaced.get("n_b", case["n_b"])
    cap = min(n_a * n_b, 40000) + 3 if cap is None else cap
    n, stats = C.c_int64(-1), (C.c_int64 * 3)(-1, -1, -1)
    head = (ptr(d_sig), ptr(d_count), n_a, replaced.get("s", case["s"]), ptr(d_ent_hash), ptr(d_ent_genome), len(case["ent_hash"]), n_b,
            replaced.get("cn", case["cn"]), replaced.get("cd", case["cd"]))
    buffer = np.full(cap * 16, 0xAB, dtype=np.uint8)
    torch.cuda.synchronize()
    if pairs_device:
        d_buffer = torch.from_numpy(buffer.copy()).to(DEVICE)
        torch.cuda.synchronize()
        code = lib.fa_screen_contained(*head, None if count_only else C.c_void_p(d_buffer.data_ptr()), cap, C.byref(n), 1, stats)
        buffer = d_buffer.cpu().numpy()
    else:
        code = lib.fa_screen_contained(*head, None if count_only else C.c_void_p(buffer.ctypes.data), cap, C.byref(n), 0, stats)
    return code, buffer, n.value, tuple(stats)


def check_contained(name, got, count_only=False):
    code, buffer, n, stats = got
    want, want_stats = expected(name)
    assert code == FA_OK, _lib.last_error()
    assert n == len(want) and stats == want_stats
    written = 0 if count_only else n * 16
    assert buffer[:written].tobytes() == want.tobytes()[:written]
    assert np.all(buffer[written:] == 0xAB)                                 # nothing is written behind the records


def untouched(got):
    return np.all(got[1] == 0xAB) and got[3] == (-1, -1, -1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_records_and_counters_match_the_restatement(name):
    assert len(expected(name)[0]) <= 40000
    check_contained(name, lib_contained(CASES[name]))
    check_contained(name, lib_contained(CASES[name], count_only=True), count_only=True)


@pytest.mark.parametrize("name", ["pool_s1000", "runs_s8", "slice_+1", "both_halves_full_s4096", "no_references_s64"])
def test_host_and_device_records_agree(name):
    check_contained(name, lib_contained(CASES[name], pairs_device=True))
    check_contained(name, lib_contained(CASES[name], pairs_device=False))


@pytest.mark.parametrize("pairs_device", [False, True])
def test_a_buffer_one_record_short_is_invalid(pairs_device):
    name = "runs_s8"
    n_records = len(expected(name)[0])
    assert n_records > 600
    got = lib_contained(CASES[name], pairs_device=pairs_device, cap=n_records - 1)
    assert got[0] == FA_ERR_INVALID and untouched(got), _lib.last_error()
    assert got[2] == n_records                                              # what the caller needs
    check_contained(name, lib_contained(CASES[name], pairs_device=pairs_device, cap=n_records))


def set_count(g, value):
    def change(sig, count, ent_hash, ent_genome):
        count[g] = value
    return change


def break_order(g, at, equal):
    def change(sig, count, ent_hash, ent_genome):
        assert count[g] > at >= 1
        sig[g, at] = sig[g, at - 1] if equal else sig[g, at - 1] - 1
    return change


def swap_hashes(last):
    """the hashes of the first (or the last) two neighbours that differ in it, the wrong way round"""
    def change(sig, count, ent_hash, ent_genome):
        at = int(np.nonzero(ent_hash[1:] != ent_hash[:-1])[0][-1 if last else 0])
        ent_hash[[at, at + 1]] = ent_hash[[at + 1, at]]
    return change


def genomes_of_a_run(descend):
    """the first two entries of a run of one hash: the same genome twice, or the two the wrong way round"""
    def change(sig, count, ent_hash, ent_genome):
        at = int(np.nonzero((ent_hash[1:] == ent_hash[:-1]))[0][0])
        ent_genome[[at, at + 1]] = ent_genome[[at + 1, at]] if descend else ent_genome[[at, at]]
    return change


def set_genome(at, value):
    def change(sig, count, ent_hash, ent_genome):
        ent_genome[at] = value
    return change


# of "pool_s1000": signatures 0, 3 and 6 are full
BAD_INPUTS = {
    "count_is_s_plus_one": set_count(2, 1001), "count_is_negative": set_count(6, -1), "count_is_huge": set_count(0, 2 ** 31 - 1),
    "a_signature_descends": break_order(0, 700, False), "a_signature_repeats_an_element": break_order(3, 1, True),
    "the_last_element_descends": break_order(6, 999, False),
    "entries_descend_by_hash": swap_hashes(False), "the_last_entries_descend": swap_hashes(True),
    "an_entry_twice": genomes_of_a_run(False), "genomes_descend_in_a_run": genomes_of_a_run(True),
    "a_genome_is_n_b": set_genome(-1, 11), "a_genome_is_negative": set_genome(0, -1), "a_genome_is_huge": set_genome(50, 2 ** 31 - 1),
}


@pytest.mark.parametrize("label", sorted(BAD_INPUTS))
def test_bad_inputs_are_invalid_and_return_nothing(label):
    name = "pool_s1000"
    assert CASES[name]["count"][[0, 3, 6]].tolist() == [1000, 1000, 1000] and CASES[name]["n_b"] == 11
    for pairs_device in (False, True):
        got = lib_contained(CASES[name], pairs_device=pairs_device, changes=BAD_INPUTS[label])
        assert got[0] == FA_ERR_INVALID and got[2] == -1 and untouched(got), (got[0], got[2], got[3], _lib.last_error())
    check_contained(name, lib_contained(CASES[name]))                       # the process goes on


def test_bad_parameters_return_nothing():
    case = CASES["pool_s64"]
    for replaced in (dict(s=0), dict(s=4097), dict(cn=-1), dict(cn=2, cd=1), dict(cd=0), dict(n_b=10), dict(n_b=-1)):
        got = lib_contained(case, cap=80, **replaced)
        assert got[0] == FA_ERR_INVALID and got[2] == -1 and untouched(got), replaced


def test_the_same_input_gives_the_same_bytes():
    for name in ("pool_s1000", "slice_+1"):
        runs = [lib_contained(CASES[name], pairs_device=True) for _ in range(3)]
        for run in runs:
            check_contained(name, run)
            assert run[1].tobytes() == runs[0][1].tobytes()


# ---- the Python face, end to end ---------------------------------------------------------------------------------------
def as_signatures(case, k=16):
    n = len(case["count"])
    return screen.Signatures(to_device(case["sig"]).view(n, -1), to_device(case["count"]), [f"q{i}" for i in range(n)], k)


def as_contents(case, k=16):
    return screen.Contents(to_device(case["ent_hash"]), to_device(case["ent_genome"]), [f"r{i}" for i in range(case["n_b"])], k)


def test_python_contained_cut_by_identity():
    case = CASES["pool_s1000"]
    sigs, contents = as_signatures(case), as_contents(case)
    assert len(contents) == 11 and contents.entries == len(case["ent_hash"])
    everything, (evaluated, _, visited) = ct.restate_contained(dict(case, cn=0, cd=1))
    sizes = []
    for cut in (0.0, 0.9, 0.97, 1.0):
        want = everything[screen.identity(everything, 16) >= cut]
        stats = {}
        got = screen.contained(sigs, contents, min_identity=cut, stats=stats)
        assert got.dtype == SCREEN_DTYPE and got.tobytes() == want.tobytes() and 0 < len(want)
        assert stats["evaluated"] == evaluated == 77 and stats["visited"] == visited and len(want) <= stats["kept"] <= len(everything)
        on_device = screen.contained(sigs, contents, min_identity=cut, device=True)
        assert on_device.is_cuda and on_device.dtype == torch.int32 and screen.to_records(on_device).tobytes() == want.tobytes()
        sizes.append(len(want))
    assert sizes[0] == len(everything) and sizes[0] > sizes[1] >= sizes[2] >= sizes[3] > 0
    with pytest.raises(ValueError, match="do not compare"):
        screen.contained(sigs, as_contents(case, k=21))
    # more records than the first buffer holds: the sizing retry
    wide = CASES["common_hash_s8"]
    want, _ = ct.restate_contained(wide)
    got = screen.contained(as_signatures(wide), as_contents(wide), min_identity=0.5)
    assert len(want) == 6400 > max(4096, 16 * 160) and got.tobytes() == want[screen.identity(want, 16) >= 0.5].tobytes() == want.tobytes()


def test_pieces_end_to_end(tmp_path):
    """Twelve genomes in three families and a 5 kb piece of member 1 of each: by the Jaccard road a piece is beyond 0.1 of every
    genome, the one it was cut from included; by containment it finds members 0, 1 and 2 of its family, nine records in all.
    Contents and records are those of the restatement on the records read back from the sketch."""
    import pyfastani_amd as pf
    genomes = sc.family_genomes()
    pieces = [genomes[4 * f + 1][20_000:25_000] for f in range(sc.FAMILIES)]
    references, queries, everything = pf.Sketch(), pf.Sketch(), pf.Sketch()
    for i, genome in enumerate(genomes):
        references.add_genome(f"genome{i}", genome)
        everything.add_genome(f"genome{i}", genome)
    for f, piece in enumerate(pieces):
        queries.add_genome(f"piece{f}", piece)
        everything.add_genome(f"piece{f}", piece)
    contents = screen.contents(references)
    assert len(contents) == 12 and contents.k == references.k == 16 and contents.names == references.names
    rec, (lengths, sbf, counter) = references._export_records("cuda")
    rec = rec.cpu().numpy()
    want_hash, want_genome = ct.restate_contents({"hash": rec[0].view(np.uint32), "seq_id": rec[1], "sbf": np.asarray(sbf, dtype=np.int32)})
    assert contents.entries == len(want_hash) > 12 * 5000
    assert contents.hash.cpu().numpy().tobytes() == want_hash.tobytes() and contents.genome.cpu().numpy().tobytes() == want_genome.tobytes()
    sigs = screen.signatures(queries, size=1000)
    count = sigs.count.cpu().numpy()
    assert len(sigs) == 3 and np.all((count > 300) & (count < 500))
    case = {"sig": sigs.sig.cpu().numpy().view(np.uint32), "count": count, "s": 1000, "ent_hash": want_hash, "ent_genome": want_genome,
            "n_b": 12, "cn": 0, "cd": 1}
    loose, _ = ct.restate_contained(case)
    stats = {}
    records = screen.contained(sigs, contents, min_identity=0.88, stats=stats)
    assert records.tobytes() == loose[screen.identity(loose, 16) >= 0.88].tobytes()
    assert [(int(r["a"]), int(r["b"])) for r in records] == [(p, 4 * p + m) for p in range(3) for m in (0, 1, 2)]        # the nine records
    assert np.all(records[1::3]["shared"] == records[1::3]["denom"]) and stats["evaluated"] == 36 and 9 <= stats["kept"] < 36
    # the Jaccard road at 0.1 keeps the families' own pairs and none with a piece in it
    jaccard = screen.pairs(screen.signatures(everything, size=1000), max_distance=0.1)
    assert len(jaccard) > 0 and np.all(jaccard["b"] < 12)
    outputs.write_containment(tmp_path / "containment.tsv", sigs.names, contents.names, records, sigs.k)
    lines = (tmp_path / "containment.tsv").read_text().splitlines()
    assert len(lines) == 9 and lines[1].startswith("piece0\tgenome1\t1\t") and lines[0].startswith("piece0\tgenome0\t0.9")
    # a collection contained in itself folds to the triangular records `groups` takes: the families
    own = screen.signatures(references, size=1000)
    folded = screen.fold(screen.contained(own, contents, min_identity=0.8))
    assert np.all(folded["a"] < folded["b"]) and screen.groups(folded, 12).tolist() == [0] * 4 + [4] * 4 + [8] * 4
