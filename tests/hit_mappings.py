"""Inputs and expected values of the hit-mapping tests (test_hit_mappings_inputs.py, test_gpu_hit_mappings.py).

The expected records are a restatement of steps 1-2 of the oracle's computeCGI (oracle/fastani_oracle.hpp:666-709, the
default FO_CGI_TIES=0 / FO_CGI_BIN=0 readings) over the oracle's full L2 mapping list:

  step 1  per (reference genome, querySeqId) the mapping of highest identity; ties to the smaller (refSeqId, refStartPos);
  step 2  per (refSeqId, bin = refStartPos // (fragment_length - 20)) the survivor of highest identity; ties to the smaller
          querySeqId;

and the records come in (reference genome, refSeqId, bin) order, the order in which step 3 sums the identities in float32.
The genome of a contig comes from sequencesByFileInfo: the cumulative number of contigs (short ones included) per genome.

Run as a program (`python hit_mappings.py CASE OUT.npz [fresh]`) it maps one input set on the GPU and stores what the device
returned; the GPU tests start it as a child process where a case needs an environment variable set before HIP starts.
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pyfastani_amd import synthetic as syn  # noqa: E402
from rules_cases import call_counters  # noqa: E402

FIELDS = ("query_id", "query_seq_id", "ref_genome_id", "ref_seq_id", "ref_start_pos", "sketch_size", "conserved", "identity")


def _draft(g, codes, n_contigs):
    return syn.split_contigs(g, syn.to_ascii(codes), n_contigs)


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
def inputs(case):
    """{"params", "refs", "queries", "sub"}: references and queries as lists of contig lists; `sub` = (first, count) or None."""
    if case == "one_part":
        # three references at d = 0.01 / 0.05 / 0.10 of a 120 kb ancestor, one query: one pass, one part, few pairs
        g = syn.rng(96)
        anc = syn.random_codes(g, 120_000)
        refs = [[syn.to_ascii(syn.mutate_codes(g, anc, d))] for d in (0.01, 0.05, 0.1)]
        queries = [[syn.to_ascii(syn.mutate_codes(g, anc, 0.03))]]
        return {"params": {}, "refs": refs, "queries": queries, "sub": None}
    if case == "contested":
        # draft references of 3 contigs, queries of 4; query 0 carries two 9 kb segments of the ancestor a second time at its
        # far end, one mutated less than the original (the late fragments win their bins) and one more (the early ones do)
        g = syn.rng(99)
        anc = syn.random_codes(g, 200_000)
        refs = [_draft(g, syn.mutate_codes(g, anc, d) if d else anc, 3) for d in (0.0, 0.02, 0.06, 0.12)]
        first = _draft(g, syn.mutate_codes(g, anc[:182_000], 0.03), 4)
        again = np.concatenate([syn.to_ascii(syn.mutate_codes(g, anc[12_000:21_000], 0.005)),
                                syn.to_ascii(syn.mutate_codes(g, anc[30_000:39_000], 0.08))])
        first[-1] = np.concatenate([first[-1][: len(first[-1]) // 3000 * 3000], again])   # (the copies start on a fragment boundary)
        queries = [first, _draft(g, syn.mutate_codes(g, anc, 0.09), 4), [syn.to_ascii(anc)]]
        return {"params": {}, "refs": refs, "queries": queries, "sub": None}
    if case == "passes":
        # 14 query genomes of 45 fragments: passes of two under FA_PASS_FRAGMENTS=120.  Query 5 is related to nothing, and
        # nothing is related to reference 5
        g = syn.rng(4142)
        ancs = [syn.random_codes(g, 135_500) for _ in range(3)]
        refs = [[syn.to_ascii(syn.mutate_codes(g, ancs[a], d))] for a, d in ((0, 0.01), (0, 0.05), (1, 0.02), (1, 0.08), (2, 0.03))]
        refs.append([syn.to_ascii(syn.random_codes(g, 135_500))])
        queries = []
        for i in range(14):
            if i == 5:
                queries.append([syn.to_ascii(syn.random_codes(g, 135_500))])
            else:
                queries.append(_draft(g, syn.mutate_codes(g, ancs[i % 3], 0.01 + 0.01 * (i % 7)), 1 + i % 2))
        return {"params": {}, "refs": refs, "queries": queries, "sub": (3, 5)}
    if case == "protein":
        golden = os.path.join(ROOT, "tests", "golden")
        b1 = _read_fasta(os.path.join(golden, "BGC0001425.faa"))
        b3 = _read_fasta(os.path.join(golden, "BGC0001428.faa"))
        return {"params": {"protein": True, "fragment_length": 100}, "refs": [b1, b1], "queries": [b3], "sub": None}
    raise KeyError(case)


CASES = ("one_part", "contested", "passes", "protein")


def fragment_length(case):
    return inputs(case)["params"].get("fragment_length", 3000)


def step1(m, sequences_by_file):
    """Indices into the oracle's mapping list of the step-1 survivors, in (genome, qseq) order, and every mapping's genome."""
    genome = np.searchsorted(np.asarray(sequences_by_file), m["rseq"], side="right")
    order = sorted(range(len(genome)), key=lambda i: (genome[i], m["qseq"][i], -m["identity"][i], m["rseq"][i], m["rstart"][i]))
    one = []
    for i in order:
        if not one or (genome[i], m["qseq"][i]) != (genome[one[-1]], m["qseq"][one[-1]]):
            one.append(i)
    return one, genome


def kept_mappings(m, sequences_by_file, frag_len, query_id=0):
    """Steps 1-2 over the oracle's mapping list `m` (OracleSketch.query_draft(..., details=True)["mappings"]): the records
    computeCGI keeps, as a MAPPING_DTYPE array in (genome, refSeqId, bin) order; also the number of step-1 survivors per genome."""
    from pyfastani_amd._batch import MAPPING_DTYPE
    one, genome = step1(m, sequences_by_file)
    bin_len = frag_len - 20
    key = lambda i: (genome[i], m["rseq"][i], m["rstart"][i] // bin_len, -m["identity"][i], m["qseq"][i])  # noqa: E731
    two = []
    for i in sorted(one, key=key):
        if not two or key(i)[:3] != key(two[-1])[:3]:
            two.append(i)
    out = np.zeros(len(two), dtype=MAPPING_DTYPE)
    for k, i in enumerate(two):
        out[k] = (query_id, m["qseq"][i], genome[i], m["rseq"][i], m["rstart"][i], m["sketch"][i], m["shared"][i], m["identity"][i])
    survivors = {}
    for i in one:
        survivors[int(genome[i])] = survivors.get(int(genome[i]), 0) + 1
    return out, survivors


def rows_of(maps):
    """Step 3 over records in the order given: [(genome, count, float32 mean of the identities summed one by one)]."""
    rows = []
    i = 0
    while i < len(maps):
        j, total = i, np.float32(0.0)
        while j < len(maps) and maps["ref_genome_id"][j] == maps["ref_genome_id"][i] and maps["query_id"][j] == maps["query_id"][i]:
            total = np.float32(total + maps["identity"][j])
            j += 1
        rows.append((int(maps["query_id"][i]), int(maps["ref_genome_id"][i]), j - i, np.float32(total / np.float32(j - i))))
        i = j
    return rows


@functools.lru_cache(maxsize=None)
def expected(case):
    """What the oracle and the restatement give for an input set, computed once per process:
    {"maps": [records per query], "survivors": [step-1 survivors per genome, per query], "orows": [oracle rows per query],
     "hits": [oracle hit list per query], "minimum_fraction"}."""
    from oracle.oracle import OracleSketch
    inp = inputs(case)
    osk = OracleSketch(**inp["params"])
    sbf, n = [], 0
    for i, contigs in enumerate(inp["refs"]):
        osk.add_draft(i, contigs)
        n += len(contigs)
        sbf.append(n)
    osk.index()
    out = {"maps": [], "survivors": [], "orows": [], "hits": []}
    for q, contigs in enumerate(inp["queries"]):
        hits, det = osk.query_draft(contigs, threads=8, details=True)
        maps, surv = kept_mappings(det["mappings"], sbf, fragment_length(case), q)
        out["maps"].append(maps)
        out["survivors"].append(surv)
        r = det["rows"]
        out["orows"].append([(int(g), int(c), np.float32(x)) for g, c, x in zip(r["genome"], r["count"], r["identity"])])
        out["hits"].append(hits)
    return out


def expected_draft(case, q=0):
    """(oracle hits of query q, the records of those hits' pairs in the hits' order)"""
    exp = expected(case)
    maps = exp["maps"][q]
    parts = [maps[maps["ref_genome_id"] == name] for name, _, _, _ in exp["hits"][q]]
    return exp["hits"][q], (np.concatenate(parts) if parts else maps[:0])


def gpu_results(case, fresh=False):
    """Maps an input set on the device: the batch's rows and mappings over the full range and the sub-range, and query 0
    through Mapper.query_draft_mappings, with the repeats and parts of each mapping call.

    A mapper learns its capacities at its first query and only ever raises them, so the void parts a lowered capacity forces
    all happen in that first call.  `fresh`: every road gets a mapper of its own and the mapping call is that mapper's FIRST
    query -- the void parts and their repeats then run with the mappings on.  Otherwise one mapper serves both roads, with
    query_draft before and after query_draft_mappings."""
    import warnings
    import pyfastani_amd as pf
    inp = inputs(case)

    def new_mapper():
        sk = pf.Sketch(**inp["params"])
        for i, contigs in enumerate(inp["refs"]):
            sk.add_draft(i, contigs)
        return sk.index()

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tup = lambda hits: np.array([(h.name, h.identity, h.matches, h.fragments) for h in hits], dtype=np.float64).reshape(-1, 4)  # noqa: E731
        out = {}
        mapper = new_mapper()
        if not fresh:
            out["hits_before"] = tup(mapper.query_draft(inp["queries"][0]))
        hits, out["draft_maps"] = mapper.query_draft_mappings(inp["queries"][0])
        out["draft_repeats"], out["draft_parts"] = call_counters(mapper)
        out["draft_hits"] = tup(hits)
        if not fresh:
            out["hits_after"] = tup(mapper.query_draft(inp["queries"][0]))
        else:
            mapper = new_mapper()
        batch = mapper.upload_genomes(inp["queries"])
        out["rows"], out["maps"] = batch.query_mappings()
        out["batch_repeats"], out["batch_parts"] = call_counters(mapper)
        out["plain_rows"] = batch.query_rows()
        if inp["sub"]:
            out["sub_rows"], out["sub_maps"] = batch.query_mappings(*inp["sub"])
            out["sub_repeats"], out["sub_parts"] = call_counters(mapper)
    return out


def check_against_expected(case, got):
    """Every assertion the GPU cases share: records field for field and in order, rows consistent with them."""
    exp = expected(case)
    inp = inputs(case)

    def same_records(a, b, what):
        assert a.dtype == b.dtype and len(a) == len(b), (what, len(a), len(b))
        if a.tobytes() != b.tobytes():
            bad = [i for i in range(len(a)) if a[i].tobytes() != b[i].tobytes()]
            raise AssertionError(f"{what}: {len(bad)} of {len(a)} records differ, first at {bad[0]}: device {a[bad[0]]} expected {b[bad[0]]}")

    def rows_match(rows, maps, what):
        want = rows_of(maps)
        have = [(int(r["query_id"]), int(r["ref_genome_id"]), int(r["count_seq"]), np.float32(r["identity"])) for r in rows]
        assert have == want, (what, have[:4], want[:4])

    want_all = np.concatenate(exp["maps"])
    same_records(got["maps"], want_all, "batch mappings")
    rows_match(got["rows"], got["maps"], "batch rows")
    assert got["rows"].tobytes() == got["plain_rows"].tobytes(), "query_mappings and query_rows return different rows"
    for q, orows in enumerate(exp["orows"]):
        have = [(int(r["ref_genome_id"]), int(r["count_seq"]), np.float32(r["identity"])) for r in got["rows"] if r["query_id"] == q]
        assert have == orows, (q, have, orows)
    if inp["sub"]:
        first, count = inp["sub"]
        same_records(got["sub_maps"], np.concatenate(exp["maps"][first:first + count]), "sub-range mappings")
        rows_match(got["sub_rows"], got["sub_maps"], "sub-range rows")
        keep = (got["rows"]["query_id"] >= first) & (got["rows"]["query_id"] < first + count)
        assert got["sub_rows"].tobytes() == got["rows"][keep].tobytes()
    hits, draft = expected_draft(case, 0)
    want_hits = np.array(hits, dtype=np.float64).reshape(-1, 4)
    for name in [n for n in ("draft_hits", "hits_before", "hits_after") if n in got]:
        assert np.array_equal(got[name], want_hits), (name, got[name], want_hits)
    same_records(got["draft_maps"], draft, "query_draft_mappings")


if __name__ == "__main__":
    case, path = sys.argv[1], sys.argv[2]
    np.savez(path, **gpu_results(case, fresh="fresh" in sys.argv[3:]))
    print("OK")
