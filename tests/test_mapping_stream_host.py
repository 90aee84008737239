"""The host side of the streamed mapping output, no GPU: the new symbols, the range planner of GenomeBatch.iter_mappings,
write_mappings(append=True), the width-agnostic record gather with all_vs_all(mappings=True) over gloo, and the window
arithmetic of csrc/fa_mapstream.h under AddressSanitizer + UBSan (scripts/host_sanitize/mapstream.cpp)."""
import ctypes as C
import os
import re
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT
from pyfastani_amd import _batch, _lib, outputs
from pyfastani_amd._batch import MAPPING_DTYPE, plan_ranges

NEW_SYMBOLS = ("fa_mapper_query_genomes_mappings_stream", "fa_mapper_query_mappings_stream", "fa_mapper_set_mapping_stage",
               "fa_mapper_mapping_memory")


def test_new_symbols_in_header_table_and_library():
    with open(os.path.join(ROOT, "include", "fastani_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*fa_mapping_sink\s*\)\s*\(\s*void\s*\*\s*user\s*,\s*const\s+fa_hit_mapping\s*\*\s*records\s*,\s*int64_t\s+n\s*\)", text)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    # the stream entries take what their buffer twins take, with (sink, user) in place of (maps, map_cap[, maps_device])
    sig = _lib.SIGNATURES
    assert sig["fa_mapper_query_genomes_mappings_stream"][1][:8] == sig["fa_mapper_query_genomes_mappings"][1][:8]
    assert sig["fa_mapper_query_mappings_stream"][1][:11] == sig["fa_mapper_query"][1]
    assert len(sig["fa_mapper_query_genomes_mappings_stream"][1]) == 11 and len(sig["fa_mapper_query_mappings_stream"][1]) == 14


def covers(ranges, first, count):
    at = first
    for lo, n in ranges:
        assert lo == at and n >= 1, (ranges, first, count)
        at += n
    assert at == first + count


@pytest.mark.parametrize("counts,per,first,count,want", [
    ([45] * 14, 120, 0, None, [(q, 2) for q in range(0, 14, 2)]),                       # even
    ([45] * 14, 120, 3, 5, [(3, 2), (5, 2), (7, 1)]),                                    # a sub-range that starts inside a pass
    ([45] * 14, 48 * 1024, 0, None, [(0, 14)]),
    ([10, 90, 20, 100, 1, 119, 1, 1], 120, 0, None, [(0, 3), (3, 2), (5, 2), (7, 1)]),   # ragged: 10+90+20, 100+1, 119+1, 1
    ([5, 500, 5, 5], 120, 0, None, [(0, 1), (1, 1), (2, 2)]),                            # a genome above the pass size is a range of its own
    ([500, 500], 120, 0, None, [(0, 1), (1, 1)]),
    ([0, 0, 50, 0, 100, 0, 0], 120, 0, None, [(0, 4), (4, 3)]),                          # empty genomes ride along
    ([0, 0, 0], 120, 0, None, [(0, 3)]),
    ([45] * 14, 120, 4, 0, []),                                                          # an empty range
    ([], 120, 0, None, []),
])
def test_plan_ranges(counts, per, first, count, want):
    got = plan_ranges(np.asarray(counts, dtype=np.uint64), per, first, count)
    n = len(counts) - first if count is None else count
    covers(got, first, n)
    assert got == want
    for lo, k in got:
        assert k == 1 or sum(counts[lo:lo + k]) <= per


def test_plan_ranges_random_and_errors():
    rng = np.random.default_rng(5)
    for _ in range(200):
        counts = rng.integers(0, 60, size=int(rng.integers(0, 30))).tolist()
        per = int(rng.integers(1, 100))
        first = int(rng.integers(0, len(counts) + 1))
        count = int(rng.integers(0, len(counts) - first + 1))
        got = plan_ranges(counts, per, first, count)
        covers(got, first, count)
        for i, (lo, k) in enumerate(got):
            assert k == 1 or sum(counts[lo:lo + k]) <= per
            if lo + k < first + count:                              # greedy: the next genome did not fit
                assert sum(counts[lo:lo + k + 1]) > per
    for bad in ((-1, 1), (0, 4), (2, 2), (0, -1)):
        with pytest.raises(ValueError):
            plan_ranges([1, 2, 3], 10, *bad)
    with pytest.raises(ValueError):
        plan_ranges([1], 0)
    assert _batch.pass_fragments() == int(os.environ.get("FA_PASS_FRAGMENTS") or 48 * 1024)


def test_write_mappings_append(tmp_path):
    maps = np.array([(0, 0, 1, 3, 5980, 120, 100, 97.5), (0, 2, 1, 3, 8940, 118, 90, 95.25), (1, 1, 0, 0, 0, 121, 121, 100.0)], dtype=MAPPING_DTYPE)
    lengths = [[9000], [3500, 3100]]
    whole, parts = tmp_path / "whole.tsv", tmp_path / "parts.tsv"
    outputs.write_mappings(whole, ["qa", "qb"], ["r0", "r1"], maps, lengths, 3000)
    outputs.write_mappings(parts, ["qa", "qb"], ["r0", "r1"], maps[:2], lengths, 3000)
    outputs.write_mappings(parts, ["qa", "qb"], ["r0", "r1"], maps[2:], lengths, 3000, append=True)
    outputs.write_mappings(parts, ["qa", "qb"], ["r0", "r1"], maps[:0], lengths, 3000, append=True)
    lines = parts.read_text().splitlines()
    assert parts.read_text() == whole.read_text()
    assert lines[0].split("\t") == list(outputs.MAPPING_COLUMNS) and len(lines) == 4
    assert sum(line.startswith("query\t") for line in lines) == 1
    # the default still starts the file afresh
    outputs.write_mappings(parts, ["qa", "qb"], ["r0", "r1"], maps[:1])
    assert len(parts.read_text().splitlines()) == 2


GATHER_WORKER = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, {root!r})
    import numpy as np, torch, torch.distributed as dist
    from pyfastani_amd import sharding
    from pyfastani_amd._batch import MAPPING_DTYPE, ROW_DTYPE
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    # (a) all_gather_records at width 5 and 8, with uneven counts and a rank that has nothing
    for width in (5, 8):
        for counts in ((3, 7), (0, 4), (5, 0), (0, 0)):
            mine = torch.arange(counts[rank] * width, dtype=torch.int32).reshape(-1, width) + 1000 * (rank + 1)
            out = sharding.all_gather_records(mine)
            want = torch.cat([torch.arange(counts[r] * width, dtype=torch.int32).reshape(-1, width) + 1000 * (r + 1) for r in range(world)])
            assert out.dtype == torch.int32 and tuple(out.shape) == (sum(counts), width) and torch.equal(out, want), (width, counts)
    # an identity travels as its bit pattern
    rec = np.array([(rank, 1, 2, 3, 4, 5, 6, np.float32(99.1234) + rank)], dtype=MAPPING_DTYPE)
    back = sharding.tensor_to_records(sharding.all_gather_records(sharding.records_to_tensor(rec, MAPPING_DTYPE)), MAPPING_DTYPE)
    assert back[rank].tobytes() == rec[0].tobytes() and len(back) == world
    # (b) all_vs_all(mappings=True) with a stand-in mapper: 7 query genomes of uneven fragment counts, 3 references; query q hits
    # reference r when (q + r) % 2 == 0, with q + 1 records whose positions rise
    frags = [30, 4, 17, 30, 2, 9, 21]
    genomes = [[b"A" * (3000 * f)] for f in frags]
    def table(q_ids):
        rows = [(local, r, q + 1, frags[q], 80.0 + q + r / 8) for local, q in enumerate(q_ids) for r in range(3) if (q + r) % 2 == 0]
        maps = [(local, k, r, r, 2980 * k, 100 + q, 90 + k, 80.0 + q + r / 8 + k / 64) for local, q in enumerate(q_ids) for r in range(3)
                if (q + r) % 2 == 0 for k in range(q + 1)]
        return (np.array(rows, dtype=ROW_DTYPE) if rows else np.zeros(0, ROW_DTYPE)), (np.array(maps, dtype=MAPPING_DTYPE) if maps else np.zeros(0, MAPPING_DTYPE))
    class Batch:
        def __init__(self, owned):
            self.owned = owned
        def query_mappings(self, first, count):
            rows, maps = table(self.owned)
            return (rows[(rows["query_id"] >= first) & (rows["query_id"] < first + count)],
                    maps[(maps["query_id"] >= first) & (maps["query_id"] < first + count)])
        def query_rows(self, first, count):
            return self.query_mappings(first, count)[0]
    class Mapper:
        fragment_length = 3000
        def upload_genomes(self, genomes):
            owned = sharding.shard_by_fragments(frags, world)[rank]
            assert len(genomes) == len(owned)
            return Batch(owned)
    want_rows, want_maps = table(list(range(7)))
    rows, maps = sharding.all_vs_all(Mapper(), genomes, rank, world, device="cpu", chunk=2, mappings=True)
    assert rows.tobytes() == want_rows.tobytes(), (rank, rows.tolist())
    assert maps.dtype == MAPPING_DTYPE and maps.tobytes() == want_maps.tobytes(), (rank, maps.tolist())
    plain = sharding.all_vs_all(Mapper(), genomes, rank, world, device="cpu", chunk=2)
    assert plain.tobytes() == want_rows.tobytes()
    dist.barrier()
    dist.destroy_process_group()
    open(os.path.join({out!r}, f"rank{{rank}}.ok"), "w").write(f"{{len(rows)}} {{len(maps)}}")
""")


def test_record_gather_and_all_vs_all_mappings_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(GATHER_WORKER.format(root=ROOT, out=str(tmp_path)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script)]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    n_rows = sum(1 for q in range(7) for r in range(3) if (q + r) % 2 == 0)
    n_maps = sum(q + 1 for q in range(7) for r in range(3) if (q + r) % 2 == 0)
    assert (tmp_path / "rank0.ok").read_text() == (tmp_path / "rank1.ok").read_text() == f"{n_rows} {n_maps}"


def test_window_arithmetic_under_sanitizers():
    """csrc/fa_mapstream.h as the kernel and the engine include it, in a program of its own under ASan + UBSan: for totals
    0..300 and stages 1..130 the windows partition [0, total) with no empty window, and the chunk predicate keeps exactly the
    chunks that hold a record of the window (brute-force model)."""
    out = os.path.join(ROOT, "build", "host_sanitize")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "mapstream_pytest")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "host_sanitize", "mapstream.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "all checks passed" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
