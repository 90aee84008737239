"""What the fragment mappings cost.
   python scripts/time_mappings.py [steps] [queries] [--stage-mb MB] [--config3 [FAMILIESxMEMBERS]] [--no-launch]

The launch leg: device time per step of a 16-query launch against the 100-reference index of the bench (config 2), with and
without mappings, the two alternating step by step.  Device time is slot [4], total_ms, of fa_mapper_last_timings (pass start to
hand-over, which follows the count, the scan and the first window of the records); the wall clock of the call also holds the
way of the records to the host, window by window through the mapping stage (--stage-mb: its size per buffer, default the
library's FA_MAP_STAGE_MB).

The config-3 leg (--config3, default 20x50 = BASELINE config 3, 1000 x 1000 genomes of 5 Mb): the whole table's mappings range
by range through GenomeBatch.iter_mappings, nothing kept but the counts: records, wall time against the plain query_rows
table, peak RSS and fa_mapper_mapping_memory.  One bounded run, not a benchmark loop."""
import argparse, sys, os, json, time, resource
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pyfastani_amd as pf
from pyfastani_amd import diagnostics, workloads

ap = argparse.ArgumentParser()
ap.add_argument("steps", nargs="?", type=int, default=10)
ap.add_argument("queries", nargs="?", type=int, default=16)
ap.add_argument("--stage-mb", default=None, help="mapping stage per buffer in MB (32 bytes per record); a comma-separated list measures "
                "each size in turn on the same mapper")
ap.add_argument("--config3", nargs="?", const="20x50", default=None, metavar="FxM", help="the config-3-shaped leg: F families of M genomes")
ap.add_argument("--length", type=int, default=5_000_000, help="genome length of the config-3 leg")
ap.add_argument("--no-launch", action="store_true", help="skip the 16 x 100 launch leg")
args = ap.parse_args()
steps, nq = args.steps, args.queries
stages_mb = [None] if args.stage_mb is None else [float(x) for x in args.stage_mb.split(",")]


def set_stage(mapper, mb):
    if mb is not None:
        mapper.set_mapping_stage(max(1, int(mb * 1024 * 1024) // 32))


def device_ms(mapper):
    ms = diagnostics.timings(mapper)
    return ms.total_ms, ms.cgi_ms


def memory(mapper):
    return dict(zip(("stage_records", "hbm_stage_bytes", "pinned_stage_bytes", "winner_table_bytes"), mapper.mapping_memory()))


def spread(a, i):
    return [round(float(np.median(a[:, i])), 4), round(float(a[:, i].min()), 4), round(float(a[:, i].max()), 4)]


def launch_leg():
    anc, names, refs = workloads.config2_references(100, 5_000_000)
    sk = pf.Sketch()
    for n, c in zip(names, refs):
        sk.add_draft(n, c)
    mapper = sk.index()
    batch = mapper.upload_genomes([workloads.config2_query(anc, 100 + i, 1)[0] for i in range(nq)])
    return [launch_steps(mapper, batch, mb) for mb in stages_mb]


def launch_steps(mapper, batch, mb):
    set_stage(mapper, mb)
    for _ in range(3):
        rows = batch.query_rows(0, nq)
        rows_m, maps = batch.query_mappings(0, nq)
    assert rows.tobytes() == rows_m.tobytes()
    assert np.array_equal(np.bincount(maps["query_id"] * 100 + maps["ref_genome_id"], minlength=nq * 100)[rows["query_id"] * 100 + rows["ref_genome_id"]], rows["count_seq"])
    plain, with_maps = [], []
    for _ in range(steps):
        t0 = time.perf_counter(); batch.query_rows(0, nq); t1 = time.perf_counter()
        plain.append(device_ms(mapper) + ((t1 - t0) * 1e3,))
        t0 = time.perf_counter(); batch.query_mappings(0, nq); t1 = time.perf_counter()
        with_maps.append(device_ms(mapper) + ((t1 - t0) * 1e3,))
    plain, with_maps = np.array(plain), np.array(with_maps)
    keys = ("device_total_ms", "cgi_stage_ms", "wall_ms")
    return {"stage_mb": mb, "queries": nq, "references": 100, "steps": steps, "rows": int(len(rows)), "mappings": int(len(maps)),
            "rows_only": {k: spread(plain, i) for i, k in enumerate(keys)},
            "with_mappings": {k: spread(with_maps, i) for i, k in enumerate(keys)},
            # what the call spends behind the device's hand-over: the records' way to the host and into the array returned
            "host_after_device_ms": {"rows_only": round(float(np.median(plain[:, 2] - plain[:, 0])), 4), "with_mappings": round(float(np.median(with_maps[:, 2] - with_maps[:, 0])), 4)},
            "memory": memory(mapper), "columns": "median, min, max over the steps"}


def config3_leg():
    fam, mem = (int(x) for x in args.config3.split("x"))
    t0 = time.perf_counter()
    genomes, _ = workloads.config3(fam, mem, args.length)
    t_gen = time.perf_counter() - t0
    n = len(genomes)
    sk = pf.Sketch()
    for i, c in enumerate(genomes):
        sk.add_draft(i, c)
    mapper = sk.index()
    batch = mapper.upload_genomes(genomes)
    del genomes, sk
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    walls, per_stage = {}, []
    for leg in ["rows_warm", "rows"] + stages_mb:
        if leg not in ("rows_warm", "rows"):
            set_stage(mapper, leg)
        t0 = time.perf_counter()
        n_rows = n_maps = n_ranges = largest = 0
        if leg not in ("rows_warm", "rows"):
            for lo, k, rows, maps in batch.iter_mappings():
                assert int(rows["count_seq"].sum()) == len(maps)
                n_rows += len(rows); n_maps += len(maps); n_ranges += 1; largest = max(largest, len(maps))
        else:
            n_rows = len(batch.query_rows())
        walls[leg] = time.perf_counter() - t0
        if leg == "rows":
            rows_plain = n_rows
        elif leg != "rows_warm":
            assert n_rows == rows_plain
            per_stage.append({"stage_mb": leg, "iter_mappings_wall_s": round(walls[leg], 4), "mappings": int(n_maps), "ranges": n_ranges,
                              "largest_range_records": int(largest), "memory": memory(mapper),
                              "peak_rss_MB": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024, 1)})
    return {"config": f"{n} x {n} ({fam} x {mem}), {args.length / 1e6:g} Mb", "generate_s": round(t_gen, 2), "rows": int(rows_plain),
            "query_rows_wall_s": round(walls["rows"], 4), "peak_rss_before_mapping_MB": round(rss0 / 1024, 1), "iter_mappings": per_stage}


out = {"stage_mb": args.stage_mb}
if not args.no_launch:
    out["launch"] = launch_leg()
if args.config3:
    out["config3"] = config3_leg()
print(json.dumps(out))
