"""What the fragment mappings cost: device time per step of a 16-query launch against the 100-reference index of the bench
(config 2), with and without mappings, the two alternating step by step:
   python scripts/time_mappings.py [steps] [queries]
Device time is slot [4] of fa_mapper_last_timings (pass start to hand-over, which follows the emission); the wall clock of
the call also holds the copy of the records to the host."""
import sys, os, json, time, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pyfastani_amd as pf
from pyfastani_amd import workloads
from pyfastani_amd._lib import lib

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
nq = int(sys.argv[2]) if len(sys.argv) > 2 else 16
anc, names, refs = workloads.config2_references(100, 5_000_000)
sk = pf.Sketch()
for n, c in zip(names, refs):
    sk.add_draft(n, c)
mapper = sk.index()
batch = mapper.upload_genomes([workloads.config2_query(anc, 100 + i, 1)[0] for i in range(nq)])


def device_ms():
    ms = (C.c_float * 24)()
    lib.fa_mapper_last_timings(mapper._h, ms, 24)
    return ms[4], ms[3]


for _ in range(3):
    rows = batch.query_rows(0, nq)
    rows_m, maps = batch.query_mappings(0, nq)
assert rows.tobytes() == rows_m.tobytes()
assert np.array_equal(np.bincount(maps["query_id"] * 100 + maps["ref_genome_id"], minlength=nq * 100)[rows["query_id"] * 100 + rows["ref_genome_id"]], rows["count_seq"])
plain, with_maps = [], []
for _ in range(steps):
    t0 = time.perf_counter(); batch.query_rows(0, nq); t1 = time.perf_counter()
    plain.append(device_ms() + ((t1 - t0) * 1e3,))
    t0 = time.perf_counter(); batch.query_mappings(0, nq); t1 = time.perf_counter()
    with_maps.append(device_ms() + ((t1 - t0) * 1e3,))
plain, with_maps = np.array(plain), np.array(with_maps)
keys = ("device_total_ms", "cgi_stage_ms", "wall_ms")
print(json.dumps({"queries": nq, "references": 100, "steps": steps, "rows": int(len(rows)), "mappings": int(len(maps)),
                  "rows_only": {k: [round(float(np.median(plain[:, i])), 4), round(float(plain[:, i].min()), 4), round(float(plain[:, i].max()), 4)] for i, k in enumerate(keys)},
                  "with_mappings": {k: [round(float(np.median(with_maps[:, i])), 4), round(float(with_maps[:, i].min()), 4), round(float(with_maps[:, i].max()), 4)] for i, k in enumerate(keys)},
                  "columns": "median, min, max over the steps"}))
