"""Inputs, oracles and expected values of the rules tests (test_rules_inputs.py, test_gpu_rules.py).

A mapper follows one reading each of three rules the reference's sources leave open (`pyfastani_amd.Rules`, fa_rules).  The
oracle of a reading is oracle/oracle.py imported with FA_ORACLE_DEFINES set to the matching FO_* switches: the module reads the
variable at import and builds a library of its own under oracle/_build/, so every reading gets a private copy of the module.

  rule                   oracle switch
  l2_confidence=0.75     FO_L2_CI=0.75f
  slide_end="fragment"   FO_SLIDE_END=1
  cgi_ties="largest"     FO_CGI_TIES=1

The cases are the smallest shapes at which each reading still moves something against the default oracle (what moves where is
asserted by test_rules_inputs.py, so that no GPU comparison passes because two readings happen to agree):

  A  ten references of 300 kb of BASELINE config 2 and its query, default parameters (w = 24)
  B  six genome-like genomes (repeats, indels, an inversion) of 300 kb, all against all: the only case with equal-identity ties
  C  A's genomes at (k, fragment) = (14, 1000), (16, 5000), (21, 3000): windows of 12, 40 and 15
  D  A's references cut into 50 contigs each and the query into 40: loci reach contig ends, where the longer slide is clamped
  E  the protein golden (w = 1): nothing moves under any reading, equality with the variant oracle is still required

`kept_mappings` restates steps 1-2 of the oracle's computeCGI (oracle/fastani_oracle.hpp:666-709) with the tie direction as a
parameter (tests/hit_mappings.py is the same restatement fixed to the default); test_rules_inputs.py checks it against the
variant oracle's rows.

Run as a program (`python rules_cases.py CASE READING OUT.npz`) it maps one case on the GPU under one reading and stores what
the device returned; the GPU tests start it as a child process where a case needs an environment variable that the library
reads once per process.
"""
import ctypes as C
import functools
import importlib.util
import os
import sys
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pyfastani_amd import synthetic as syn, workloads  # noqa: E402

READINGS = {
    "default": {},
    "ci": {"l2_confidence": 0.75},
    "end": {"slide_end": "fragment"},
    "ties": {"cgi_ties": "largest"},
    "all": {"l2_confidence": 0.75, "slide_end": "fragment", "cgi_ties": "largest"},
}
SWITCHES = {"l2_confidence": "FO_L2_CI=0.75f", "slide_end": "FO_SLIDE_END=1", "cgi_ties": "FO_CGI_TIES=1"}
CASES = ("A", "B", "C", "D", "E")
# the readings the GPU test runs per case: each single one and all three together on A-D, all three together on E
GPU_READINGS = {c: ("ci", "end", "ties", "all") for c in "ABCD"}
GPU_READINGS["E"] = ("all",)


def defines(reading):
    return ",".join(SWITCHES[k] for k in ("l2_confidence", "slide_end", "cgi_ties") if k in READINGS[reading])


# ---- the oracle of a reading --------------------------------------------------------------------------------------------
_oracles = {}


def _load_oracle(reading):
    if reading not in _oracles:
        old = os.environ.get("FA_ORACLE_DEFINES")
        os.environ["FA_ORACLE_DEFINES"] = defines(reading)
        try:
            spec = importlib.util.spec_from_file_location(f"_oracle_{reading}", os.path.join(ROOT, "oracle", "oracle.py"))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)                     # (reads FA_ORACLE_DEFINES here, and only here)
        finally:
            if old is None:
                del os.environ["FA_ORACLE_DEFINES"]
            else:
                os.environ["FA_ORACLE_DEFINES"] = old
        _oracles[reading] = mod
    return _oracles[reading]


def oracle(reading):
    """The private copy of oracle/oracle.py of a reading, its library built (all the libraries still missing are compiled at
    once, side by side: a fresh checkout pays for one compilation, not five)."""
    mods = [_load_oracle(r) for r in READINGS]
    missing = [m for m in mods if not os.path.exists(m._SO)]
    if missing:
        with ThreadPoolExecutor(len(missing)) as pool:
            list(pool.map(lambda m: m.build(), missing))
    mod = _oracles[reading]
    mod.build()
    return mod


# ---- inputs -------------------------------------------------------------------------------------------------------------
def _read_fasta(path):
    records, cur = [], None
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                cur = []
                records.append(cur)
            elif line and cur is not None:
                cur.append(line)
    return ["".join(r) for r in records]


@functools.lru_cache(maxsize=None)
def _config2():
    anc, _, refs = workloads.config2_references(10, 300_000)
    return refs, workloads.config2_query(anc)[0]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The cells of a case: [{"params", "refs", "queries"}], references and queries as lists of contig lists."""
    if case == "A":
        refs, query = _config2()
        return [{"params": {}, "refs": refs, "queries": [query]}]
    if case == "B":
        genomes, _ = workloads.genome_like(6000, 2, 3, 300_000, inversion=30_000)
        return [{"params": {}, "refs": genomes, "queries": genomes}]
    if case == "C":
        refs, query = _config2()
        return [{"params": {"k": k, "fragment_length": frag}, "refs": refs, "queries": [query]} for k, frag in ((14, 1000), (16, 5000), (21, 3000))]
    if case == "D":
        refs, query = _config2()
        return [{"params": {}, "refs": [syn.split_contigs(syn.rng(77), r[0], 50) for r in refs],
                 "queries": [syn.split_contigs(syn.rng(77), query[0], 40)]}]
    if case == "E":
        golden = os.path.join(ROOT, "tests", "golden")
        b1 = _read_fasta(os.path.join(golden, "BGC0001425.faa"))
        b3 = _read_fasta(os.path.join(golden, "BGC0001428.faa"))
        return [{"params": {"protein": True, "fragment_length": 100}, "refs": [b1, b1], "queries": [b3]}]
    raise KeyError(case)


def fragment_length(cell):
    return cell["params"].get("fragment_length", 3000)


# ---- computeCGI, steps 1-2, with the tie direction as a parameter -----------------------------------------------------------
def kept_mappings(m, sequences_by_file, frag_len, largest, query_id=0):
    """The records computeCGI keeps of the oracle's mapping list `m` (OracleSketch.query_draft(..., details=True)["mappings"]),
    as a MAPPING_DTYPE array in (genome, refSeqId, bin) order -- the order in which step 3 sums the identities in float32:

      step 1  per (reference genome, querySeqId) the mapping of highest identity; ties to the smallest (refSeqId, refStartPos),
              or to the largest;
      step 2  per (refSeqId, bin = refStartPos // (fragment_length - 20)) the survivor of highest identity; ties to the
              smallest querySeqId, or to the largest."""
    from pyfastani_amd._batch import MAPPING_DTYPE
    sign = -1 if largest else 1
    genome = np.searchsorted(np.asarray(sequences_by_file), m["rseq"], side="right")
    order = sorted(range(len(genome)), key=lambda i: (genome[i], m["qseq"][i], -m["identity"][i], sign * m["rseq"][i], sign * m["rstart"][i]))
    one = []
    for i in order:
        if not one or (genome[i], m["qseq"][i]) != (genome[one[-1]], m["qseq"][one[-1]]):
            one.append(i)
    bin_len = frag_len - 20
    key = lambda i: (genome[i], m["rseq"][i], m["rstart"][i] // bin_len, -m["identity"][i], sign * m["qseq"][i])  # noqa: E731
    two = []
    for i in sorted(one, key=key):
        if not two or key(i)[:3] != key(two[-1])[:3]:
            two.append(i)
    out = np.zeros(len(two), dtype=MAPPING_DTYPE)
    for k, i in enumerate(two):
        out[k] = (query_id, m["qseq"][i], genome[i], m["rseq"][i], m["rstart"][i], m["sketch"][i], m["shared"][i], m["identity"][i])
    return out


def rows_of(maps):
    """Step 3 over records in the order given: [(genome, count, float32 mean of the identities summed one by one)] per query."""
    rows, i = [], 0
    while i < len(maps):
        j, total = i, np.float32(0.0)
        while j < len(maps) and maps["ref_genome_id"][j] == maps["ref_genome_id"][i] and maps["query_id"][j] == maps["query_id"][i]:
            total = np.float32(total + maps["identity"][j])
            j += 1
        rows.append((int(maps["ref_genome_id"][i]), j - i, np.float32(total / np.float32(j - i))))
        i = j
    return rows


# ---- expected values ----------------------------------------------------------------------------------------------------
def expected_cell(cell, reading):
    """What the oracle of a reading gives for one cell {"params", "refs", "queries"}: per query
    {"hits", "l2": every L2 mapping (qseq, rseq, rstart, sketch, shared), sorted, "rows": [(genome, count, float32 identity)],
     "kept": the records of the restated computeCGI under the reading's tie direction}."""
    mod = oracle(reading)
    largest = READINGS[reading].get("cgi_ties") == "largest"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        osk = mod.OracleSketch(**cell["params"])
    sbf, n = [], 0
    for i, contigs in enumerate(cell["refs"]):
        osk.add_draft(i, contigs)
        n += len(contigs)
        sbf.append(n)
    osk.index()
    per_query = []
    for q, contigs in enumerate(cell["queries"]):
        hits, det = osk.query_draft(contigs, threads=8, details=True)
        m, r = det["mappings"], det["rows"]
        per_query.append({
            "hits": hits,
            "l2": sorted(zip(m["qseq"].tolist(), m["rseq"].tolist(), m["rstart"].tolist(), m["sketch"].tolist(), m["shared"].tolist())),
            "rows": [(int(g), int(c), np.float32(x)) for g, c, x in zip(r["genome"], r["count"], r["identity"])],
            "kept": kept_mappings(m, sbf, fragment_length(cell), largest, q),
        })
    return per_query


@functools.lru_cache(maxsize=None)
def expected(case, reading):
    """`expected_cell` of every cell of a case, computed once per process."""
    return [expected_cell(cell, reading) for cell in inputs(case)]


def moved_between(a, b):
    """What differs between two answers of the form of `expected` (per cell, per query), summed over cells and queries:
    {"l2": mappings (as multisets), "rows": rows, "hits": queries whose hit list differs}."""
    from collections import Counter
    out = {"l2": 0, "rows": 0, "hits": 0, "l2_per_cell": [], "rows_per_cell": []}
    for ca, cb in zip(a, b):
        l2 = rows = 0
        for qa, qb in zip(ca, cb):
            ma, mb = Counter(qa["l2"]), Counter(qb["l2"])
            l2 += max(sum((ma - mb).values()), sum((mb - ma).values()))
            ra, rb = {r[0]: r for r in qa["rows"]}, {r[0]: r for r in qb["rows"]}
            rows += sum(ra[g] != rb[g] for g in set(ra) & set(rb)) + len(set(ra) ^ set(rb))
            out["hits"] += qa["hits"] != qb["hits"]
        out["l2"] += l2
        out["rows"] += rows
        out["l2_per_cell"].append(l2)
        out["rows_per_cell"].append(rows)
    return out


def moved(case, reading):
    """What a reading moves against the default oracle in a case (`moved_between`)."""
    return moved_between(expected(case, "default"), expected(case, reading))


def oracle_upper(olib, c, s, k, ci):
    """nucIdentityUpperBound of c shared records of a sketch of s at interval ci, by the oracle's doL2Mapping arithmetic (float32
    throughout)."""
    md = olib.fo_j2md(np.float32(c / s), k)
    lower = np.float32(olib.fo_md_lower_bound(md, s, k, ci))
    return np.float32(100) * (np.float32(1) - lower)


def oracle_threshold(olib, s, k, pid, ci):
    """Smallest shared count whose upper-bound identity passes (s + 1: none does)."""
    for c in range(s + 1):
        if oracle_upper(olib, c, s, k, ci) >= np.float32(pid):
            return c
    return s + 1


# ---- the device side ------------------------------------------------------------------------------------------------------
def gpu_l2(mapper):
    """Every L2 mapping of the mapper's last query call (one query genome: the fragment number is its querySeqId), sorted; None
    when the call ran in more parts than the stage getters keep."""
    from pyfastani_amd import _lib
    cap = 1 << 20
    buf = (_lib.Mapping * cap)()
    n = C.c_int64(0)
    try:
        _lib.check(_lib.lib.fa_mapper_debug_mappings(mapper._h, buf, cap, C.byref(n)))
    except (RuntimeError, NotImplementedError) as e:
        if "stage getters" not in str(e):
            raise
        return None
    assert n.value <= cap
    return sorted((buf[i].query_seq_id, buf[i].ref_seq_id, buf[i].ref_start_pos, buf[i].sketch_size, buf[i].conserved) for i in range(n.value))


def new_mapper(cell, reading="default"):
    import pyfastani_amd as pf
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk = pf.Sketch(**cell["params"], rules=pf.Rules(**READINGS[reading]) if reading != "default" else None)
        for i, contigs in enumerate(cell["refs"]):
            sk.add_draft(i, contigs)
        return sk.index()


def hit_tuples(hits):
    return [(h.name, h.identity, h.matches, h.fragments) for h in hits]


def gpu_cell(mapper, cell):
    """Per query of a cell, under the rules the mapper holds: {"hits", "l2", "rows", "kept"} in the form of `expected` (the rows
    and the records they are made of from one call, the L2 mappings from the stage getters behind it)."""
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        batch = mapper.upload_genomes(cell["queries"])
        for q, contigs in enumerate(cell["queries"]):
            rows, kept = batch.query_mappings(q, 1)
            l2 = gpu_l2(mapper)
            out.append({"hits": hit_tuples(mapper.query_draft(contigs)), "l2": l2, "kept": kept,
                        "rows": [(int(r["ref_genome_id"]), int(r["count_seq"]), np.float32(r["identity"])) for r in rows]})
    return out


def assert_same(got, want, what, in_parts=False):
    """L2 mappings field for field, rows with count and float32 identity bit-equal, the hit list, and the records behind the rows
    against the restated computeCGI.  `in_parts`: the call was forced into parts, of which the stage getters keep the last only;
    the records (position and shared count of every mapping that computeCGI kept) then stand for the L2 list."""
    assert len(got) == len(want), what
    for q, (g, w) in enumerate(zip(got, want)):
        assert (g["l2"] is None) == in_parts, (what, q)
        assert g["kept"].dtype == w["kept"].dtype and g["kept"].tobytes() == w["kept"].tobytes(), (what, q, len(g["kept"]), len(w["kept"]))
        if not in_parts and g["l2"] != w["l2"]:
            sg, sw = set(g["l2"]), set(w["l2"])
            raise AssertionError(f"{what}, query {q}: L2 mappings differ (device {len(g['l2'])}, oracle {len(w['l2'])}); "
                                 f"only device {sorted(sg - sw)[:4]}, only oracle {sorted(sw - sg)[:4]}")
        assert [(a, b, np.float32(c).tobytes()) for a, b, c in g["rows"]] == [(a, b, np.float32(c).tobytes()) for a, b, c in w["rows"]], \
            (what, q, g["rows"][:4], w["rows"][:4])
        assert g["hits"] == w["hits"], (what, q, g["hits"][:4], w["hits"][:4])


def pack(results):
    """The result of `gpu_cell` for several cells as arrays (for a child process to store)."""
    out = {}
    for c, per_query in enumerate(results):
        for q, r in enumerate(per_query):
            out[f"l2_{c}_{q}"] = np.asarray(r["l2"] or [], dtype=np.int64).reshape(-1, 5)
            out[f"l2_missing_{c}_{q}"] = np.asarray(r["l2"] is None)
            out[f"kept_{c}_{q}"] = r["kept"]
            out[f"rows_{c}_{q}"] = np.asarray([(g, n, np.float32(x).view(np.uint32)) for g, n, x in r["rows"]], dtype=np.int64).reshape(-1, 3)
            out[f"hits_{c}_{q}"] = np.asarray(r["hits"], dtype=np.float64).reshape(-1, 4)
    return out


def unpack(z, cells):
    """The inverse of `pack` for the cells that were mapped (e.g. `inputs(case)`)."""
    out = []
    for c, cell in enumerate(cells):
        per_query = []
        for q in range(len(cell["queries"])):
            per_query.append({
                "l2": None if bool(z[f"l2_missing_{c}_{q}"]) else [tuple(int(v) for v in row) for row in z[f"l2_{c}_{q}"]],
                "kept": z[f"kept_{c}_{q}"],
                "rows": [(int(g), int(n), np.uint32(x).view(np.float32)) for g, n, x in z[f"rows_{c}_{q}"]],
                "hits": [(int(h[0]), float(h[1]), int(h[2]), int(h[3])) for h in z[f"hits_{c}_{q}"]],
            })
        out.append(per_query)
    return out


def call_counters(mapper):
    """(repeated attempts, accepted parts) of the mapper's most recent query call: speculation misses; parts whose sketch stage
    ran fused / as two kernels."""
    from pyfastani_amd import diagnostics
    ms = diagnostics.timings(mapper)
    return int(ms.repeats), int(ms.fused + ms.unfused)


if __name__ == "__main__":
    case_, reading_, path_ = sys.argv[1], sys.argv[2], sys.argv[3]
    results_, repeats_, parts_ = [], 0, 0
    for cell_ in inputs(case_):
        mapper_ = new_mapper(cell_, reading_)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            first_ = mapper_.upload_genomes(cell_["queries"][:1]).query_rows(0, 1)     # the mapper's first call: where capacities are learnt
        r_, p_ = call_counters(mapper_)
        repeats_ += r_
        parts_ += p_
        results_.append(gpu_cell(mapper_, cell_))
    np.savez(path_, repeats=repeats_, parts=parts_, **pack(results_))
    print("OK")
