"""Differential fuzzing of the HIP path against the CPU oracle: random genomes with planted repeats, tandem
duplications, inversions, N runs and low-complexity stretches; random parameters.  Every L2 mapping and every hit must
match.  Usage: python scripts/fuzz_parity.py [--rules l2_confidence=0.75,slide_end=fragment,cgi_ties=largest] [--history | --domain | --contigs | --kmers] [cases] [seed] [seconds] [default-cell]   (stops after `seconds` if given: a
time box; a fourth argument keeps every nucleotide case in the default cell k = 16 / fragment 3000 / 80 % with queries of plain
ACGT -- the cell whose query passes run K1 and the fragment sketch as ONE launch, k_query_fused).  --history: one index per
case, then 4-8 queries drawn from the generators (plain, tandem, drafts, N / IUPAC, batches) on the SAME mapper, each through
a random entry point (query_draft, query_genome, GenomeBatch.query(first, count), query_fasta_stream), each compared with the
oracle: a mapper's speculation record carries the sizes and kernel forms of one query into the next.  --domain: the ends of
the window range -- percentage_identity from 64.5-70 (w = 2-4) and 96-100 (sketches of a handful of records), p_value from
1e-1 to 1e-12, k from 5 to 33.  --contigs: references and queries cut into 1-400 contigs by tests/contig_domain.py's cut_at at the
case's own critical lengths (0, 1, k - 1 ... k + w + 1, cmw, fragment - 1 / + 0 / + 1, two fragments, the tile seams), half of the genomes with repeats inside
their contigs (plant_repeats), with a 30 % chance each of a genome without a contig and of a genome of contigs too short for a record; batches as in the default mode.
--kmers: k from the critical list of tests/kmer_domain.py (KS, 1 to 2048) and from 1..64, an EXPLICIT window from its WS (one per form of K1; the recommended
window is the fragment itself from about k = 22 on), genomes by the rules of that module's end-to-end cells: 12 kb within 0.4 % up to k = 7, 40 kb
within 0.4 % up to k = 100, 40 kb within 0.03 % beyond, where the fragment grows to 5000 once k + w leaves fewer than 500 windows in 3000."""
import sys, os, ctypes as C, warnings, time, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pyfastani_amd as pf
from pyfastani_amd import _lib, synthetic as syn
from pyfastani_amd._lib import lib, check

# --rules l2_confidence=0.75,slide_end=fragment,cgi_ties=largest (any subset): every sketch of the run gets these rules, and the
# oracle is built with the matching FO_* switches -- oracle.oracle reads FA_ORACLE_DEFINES when it is imported, hence before it
RULES = None
if "--rules" in sys.argv:
    at = sys.argv.index("--rules")
    spec = dict(item.split("=", 1) for item in sys.argv[at + 1].split(",") if item)
    del sys.argv[at: at + 2]
    if "l2_confidence" in spec:
        spec["l2_confidence"] = float(spec["l2_confidence"])
    RULES = pf.Rules(**spec)
    switches = []
    if RULES.l2_confidence != 0.9:
        switches.append(f"FO_L2_CI={RULES.l2_confidence!r}f")
    if RULES.slide_end == "fragment":
        switches.append("FO_SLIDE_END=1")
    if RULES.cgi_ties == "largest":
        switches.append("FO_CGI_TIES=1")
    os.environ["FA_ORACLE_DEFINES"] = ",".join(switches)
from oracle.oracle import OracleSketch

def mappings(mapper):
    cap = 1 << 20
    buf = (_lib.Mapping * cap)(); n = C.c_int64(0)
    check(lib.fa_mapper_debug_mappings(mapper._h, buf, cap, C.byref(n)))
    return sorted((buf[i].query_seq_id, buf[i].ref_seq_id, buf[i].ref_start_pos, buf[i].sketch_size, buf[i].conserved) for i in range(n.value))

def scramble(g, codes):
    """plant structure: tandem repeats, a dispersed repeat, an inversion, a low-complexity run"""
    c = codes.copy()
    n = len(c)
    if g.random() < 0.7:
        unit = syn.random_codes(g, int(g.integers(20, 400)))
        p = int(g.integers(0, n - 5000)); reps = int(g.integers(2, 12))
        block = np.tile(unit, reps)[: n - p - 1]
        c[p:p + len(block)] = block
    if g.random() < 0.7:
        rep = syn.random_codes(g, int(g.integers(100, 1500)))
        for _ in range(int(g.integers(2, 6))):
            p = int(g.integers(0, n - len(rep) - 1)); c[p:p + len(rep)] = rep
    if g.random() < 0.5:
        a = int(g.integers(0, n - 4000)); b = a + int(g.integers(500, 3500))
        c[a:b] = syn.reverse_complement_codes(c[a:b])
    if g.random() < 0.5:
        p = int(g.integers(0, n - 600)); c[p:p + int(g.integers(50, 500))] = int(g.integers(0, 4))
    if g.random() < 0.4:
        p = int(g.integers(0, n - 600)); L = int(g.integers(20, 300)); c[p:p + L] = np.tile(np.array([0, 3], dtype=np.uint8), L)[:L]
    return c

def to_bytes(g, codes):
    b = bytearray(bytes(syn.to_ascii(codes)))
    if len(b) < 2500:
        return bytes(b)
    if g.random() < 0.5:
        for _ in range(int(g.integers(1, 5))):
            p = int(g.integers(0, len(b) - 200)); L = int(g.integers(1, 150)); b[p:p + L] = b"N" * L
    if g.random() < 0.3:
        p = int(g.integers(0, len(b) - 10)); b[p:p + 5] = b"RYKMS"
    if g.random() < 0.3:
        p = int(g.integers(0, len(b) - 2000)); b[p:p + 1000] = bytes(b[p:p + 1000]).lower()
    return bytes(b)

history = "--history" in sys.argv
if history:
    sys.argv.remove("--history")
domain = "--domain" in sys.argv
if domain:
    sys.argv.remove("--domain")
contig_mode = "--contigs" in sys.argv
if contig_mode:
    sys.argv.remove("--contigs")
    # the generator lives beside the tests that share it; the other modes do not need it
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import contig_domain as cd
kmer_mode = "--kmers" in sys.argv
if kmer_mode:
    sys.argv.remove("--kmers")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import kmer_domain as kd
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 50
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
time_box = float(sys.argv[3]) if len(sys.argv) > 3 else 0.0
default_cell = len(sys.argv) > 4
done = 0
g = syn.rng(seed)
bad = 0
degenerate = 0
t0 = time.time()
AMINO = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)

def protein_case(g, case):
    k = int(g.choice([5, 7, 9, 12, 16])); frag = int(g.choice([60, 100, 150, 300]))
    params = dict(k=k, fragment_length=frag, protein=True, minimum_fraction=float(g.choice([0.0, 0.2])))
    sk, osk = pf.Sketch(**params, rules=RULES), OracleSketch(**params)
    n_prot = int(g.integers(3, 12))
    anc = [g.integers(0, 20, int(g.integers(80, 900))) for _ in range(n_prot)]
    def mutate(p, d):
        p = p.copy(); m = g.random(len(p)) < d; p[m] = g.integers(0, 20, int(m.sum())); return p
    for i in range(int(g.integers(1, 4))):
        d = float(g.choice([0.0, 0.05, 0.15, 0.3]))
        prots = [bytes(AMINO[mutate(p, d)]) for p in anc]
        if g.random() < 0.3: prots.append(b"MK")
        sk.add_draft(i, prots); osk.add_draft(i, prots)
    mapper = sk.index(); osk.index()
    query = [bytes(AMINO[mutate(p, 0.08)]).lower() if g.random() < 0.2 else bytes(AMINO[mutate(p, 0.08)]) for p in anc]
    hits = [(h.name, h.identity, h.matches, h.fragments) for h in mapper.query_draft(query)]
    ohits, det = osk.query_draft(query, threads=4, details=True)
    om = det["mappings"]
    omm = sorted(zip(om["qseq"].tolist(), om["rseq"].tolist(), om["rstart"].tolist(), om["sketch"].tolist(), om["shared"].tolist()))
    try:
        gm = mappings(mapper)
    except (RuntimeError, NotImplementedError) as e:
        if "stage getters" not in str(e):
            raise
        gm = omm
    ok = hits == ohits and gm == omm and len(mapper.lookup_index) == osk.index_size
    if not ok:
        print(f"MISMATCH protein case {case} seed {seed} params {params}: {hits} vs {ohits}")
    return ok

def hit_list(hits):
    return [(h.name, h.identity, h.matches, h.fragments) for h in hits]

def history_case(g, case, tmp):
    """One index, then 4-8 queries of every kind through random entry points on the same mapper, each against the oracle."""
    k = int(g.choice([11, 14, 16, 16, 16, 21])); frag = int(g.choice([500, 1000, 3000, 3000, 5000]))
    params = dict(k=k, fragment_length=frag, percentage_identity=float(g.choice([75, 80, 80, 90])), minimum_fraction=float(g.choice([0.0, 0.2])))
    osk = OracleSketch(**params)
    if osk.window_size >= frag:
        return True
    sk = pf.Sketch(**params, rules=RULES)
    length = int(g.integers(max(3 * frag, 8000), 60_000))
    anc = scramble(g, syn.random_codes(g, length))
    copies = int(g.choice([1, 1, 2, 8, 30]))                   # many copies of one genome: fragments with thousands of seed hits
    n_ref = int(g.integers(1, 5))
    for i in range(n_ref + copies - 1):
        d = float(g.choice([0.0, 0.01, 0.03, 0.06, 0.1])) if i < n_ref else 0.0
        r = scramble(g, syn.mutate_codes(g, anc, d)) if g.random() < 0.5 and i < n_ref else syn.mutate_codes(g, anc, d)
        contigs = [to_bytes(g, x) for x in syn.split_contigs(g, r, int(g.integers(1, 4)))]
        sk.add_draft(i, contigs); osk.add_draft(i, contigs)
    other = syn.random_codes(g, length)
    r = to_bytes(g, other); sk.add_draft("u", [r]); osk.add_draft("u", [r])
    mapper = sk.index(); osk.index()

    def make_query():
        kind = str(g.choice(["plain", "tandem", "draft", "dirty", "other"]))
        src = other if kind == "other" else anc
        c = syn.mutate_codes(g, src, float(g.choice([0.0, 0.02, 0.05, 0.1])))
        if kind == "tandem":
            unit = c[: int(g.integers(200, 2 * frag))]
            c = np.concatenate([syn.mutate_codes(g, unit, 0.01) for _ in range(max(2, length // (3 * len(unit))))])
        elif kind != "plain":
            c = scramble(g, c)
        pieces = syn.split_contigs(g, c, int(g.integers(2, 6))) if kind == "draft" else [c]
        return [to_bytes(g, x) if kind == "dirty" else bytes(syn.to_ascii(x)) for x in pieces]

    ok = True
    for step in range(int(g.integers(4, 9))):
        entry = str(g.choice(["draft", "genome", "batch", "stream"]))
        queries = [make_query() for _ in range(int(g.integers(2, 5)) if entry in ("batch", "stream") else 1)]
        if entry == "genome" and len(queries[0]) > 1:
            entry = "draft"
        if entry == "draft":
            got = [hit_list(mapper.query_draft(queries[0]))]
        elif entry == "genome":
            got = [hit_list(mapper.query_genome(queries[0][0]))]
        elif entry == "batch":
            first = int(g.integers(0, len(queries))); count = int(g.integers(1, len(queries) - first + 1))
            got = [hit_list(h) for h in mapper.upload_genomes(queries).query(first, count)]
            queries = queries[first: first + count]
        else:
            paths = []
            for j, q in enumerate(queries):
                paths.append(os.path.join(tmp, f"q{step}_{j}.fa"))
                with open(paths[-1], "wb") as f:
                    f.write(b"".join(b">c%d\n" % i + x + b"\n" for i, x in enumerate(q)))
            got = [None] * len(queries)
            for first, res in mapper.query_fasta_stream(paths):
                for j, h in enumerate(res):
                    got[first + j] = hit_list(h)
        want = [osk.query_draft(q, threads=8) for q in queries]
        if got != want:
            ok = False
            print(f"MISMATCH history case {case} step {step} ({entry}) seed {seed} params {params} copies {copies}: {got} vs {want}")
    return ok

def contigs_case(g, case):
    """Fragmented references and queries at the case's own critical lengths; one query through query_draft (hits, every L2
    mapping, index size, threshold) or, every fourth case, 1-3 queries as a resident batch."""
    k = int(g.choice([11, 14, 16, 16, 16, 21])); frag = int(g.choice([200, 500, 1000, 3000, 3000]))
    params = dict(k=k, fragment_length=frag, percentage_identity=float(g.choice([75, 80, 80, 85])), minimum_fraction=float(g.choice([0.0, 0.2, 0.5])))
    osk = OracleSketch(**params)
    w = osk.window_size
    if w >= frag:
        return None
    sk = pf.Sketch(**params, rules=RULES)
    lengths = cd.critical_lengths(k, w, frag, (cd.k1_tile_len(w),) + cd.FORCED_TILES)

    def cut(codes, filler):
        seq = to_bytes(g, codes) if g.random() < 0.3 else bytes(syn.to_ascii(codes))
        if g.random() < 0.15:
            return [seq]
        at = int(g.integers(0, len(lengths)))
        contigs = cd.cut_at(g, seq, lengths[at:] + lengths[:at], filler)
        if g.random() < 0.5:
            contigs = cd.plant_repeats(contigs, k, w, frag)      # the same hash twice inside a contig: rec_prev and the linked flags
        return contigs[:399] + [b"".join(contigs[399:])] if len(contigs) > 400 else contigs

    def odd_genomes():
        out = []
        if g.random() < 0.3:
            out.append([])
        if g.random() < 0.3:
            out.append([bytes(syn.to_ascii(syn.random_codes(g, int(g.integers(0, min(k, w)))))) for _ in range(int(g.integers(1, 6)))])
        return out

    length = int(g.integers(max(12 * frag, 15_000), 120_000))
    anc = scramble(g, syn.random_codes(g, length)) if g.random() < 0.5 else syn.random_codes(g, length)
    refs = [cut(syn.mutate_codes(g, anc, float(g.choice([0.0, 0.01, 0.03, 0.06, 0.1]))), cd.ref_filler(k, w, frag)) for _ in range(int(g.integers(1, 5)))]
    if g.random() < 0.5:
        refs.append([bytes(syn.to_ascii(syn.random_codes(g, length // 2)))])
    for odd in odd_genomes():
        refs.insert(int(g.integers(0, len(refs) + 1)), odd)
    for i, contigs in enumerate(refs):
        sk.add_draft(i, contigs); osk.add_draft(i, contigs)
    mapper = sk.index(); osk.index()
    queries = [cut(syn.mutate_codes(g, anc, float(g.choice([0.0, 0.02, 0.05, 0.1]))), cd.query_filler(k, w, frag))
               for _ in range(int(g.integers(1, 4)) if case % 4 == 0 else 1)]
    ok = len(mapper.lookup_index) == osk.index_size and mapper.occurences_threshold == osk.freq_threshold
    if len(queries) > 1:
        for odd in odd_genomes():
            queries.insert(int(g.integers(0, len(queries) + 1)), odd)
        got = [hit_list(hs) for hs in mapper.upload_genomes(queries).query()]
        want = [osk.query_draft(q, threads=8) for q in queries]
        ok = ok and got == want
        if not ok:
            print(f"MISMATCH contigs batch case {case} seed {seed} params {params}: {got} vs {want}")
        return ok
    hits = hit_list(mapper.query_draft(queries[0]))
    ohits, det = osk.query_draft(queries[0], threads=8, details=True)
    omm = cd.mapping_tuples(det)
    try:
        gm = mappings(mapper)
    except (RuntimeError, NotImplementedError) as e:   # only a pass forced into parts may leave the stage getters without its mappings
        if "stage getters" not in str(e) or not os.environ.get("FA_PASS_FRAGMENTS"):
            raise
        gm = omm
    ok = ok and hits == ohits and gm == omm
    if not ok:
        print(f"MISMATCH contigs case {case} seed {seed} params {params} window {w} contigs {[len(r) for r in refs]} / {len(queries[0])}: "
              f"hits {hits} vs {ohits}; mappings gpu {len(gm)} oracle {len(omm)}")
        sg, so = set(gm), set(omm)
        print("   only gpu", sorted(sg - so)[:4], "only oracle", sorted(so - sg)[:4])
    return ok

def kmers_case(g, case):
    """One (k, w) with an explicit window; one query through query_draft (hits, every L2 mapping, index size, threshold) or,
    every fourth case, two queries as a resident batch.  None: the oracle maps nothing."""
    k = int(g.choice(kd.KS)) if g.random() < 0.5 else int(g.integers(1, 65))
    # (windows 1 and 2 at small k: every fragment would gather more than 8 192 seed hits inside one contig, the oversized-seed
    # road that tests/kmer_domain.py keeps its cells away from)
    w = int(g.choice([x for x in kd.WS if x >= (4 if k < 10 else 1)]))
    frag = 3000 if k + w + 500 <= 3000 else 5000
    length = 12_000 if k <= 7 else 40_000
    divergences = [0.001, 0.004, 0.002] if k <= 100 else [0.0, 0.0001, 0.0003]
    sk, osk = kd.sketch_pair(k, w, frag, float(g.choice([0.0, 0.2])), rules=RULES)
    anc = syn.random_codes(g, length)
    refs = [[bytes(x) for x in syn.split_contigs(g, syn.to_ascii(syn.mutate_codes(g, anc, d)), int(g.integers(1, 4)))] for d in divergences[: int(g.integers(1, 4))]]
    if g.random() < 0.5:
        refs.append([bytes(syn.to_ascii(syn.random_codes(g, length // 2)))])
    for i, contigs in enumerate(refs):
        sk.add_draft(i, contigs); osk.add_draft(i, contigs)
    mapper = sk.index(); osk.index()
    ok = len(mapper.lookup_index) == osk.index_size and mapper.occurences_threshold == osk.freq_threshold
    dq = divergences[1] if k > 100 else 0.003
    queries = [[bytes(x) for x in syn.split_contigs(g, syn.to_ascii(syn.mutate_codes(g, anc, dq)), int(g.integers(1, 4)))] for _ in range(2 if case % 4 == 0 else 1)]
    if len(queries) > 1:
        got = [hit_list(hs) for hs in mapper.upload_genomes(queries).query()]
        want = [osk.query_draft(q, threads=8) for q in queries]
        if not (ok and got == want):
            print(f"MISMATCH kmers batch case {case} seed {seed} k {k} w {w} fragment {frag}: {got} vs {want}")
            return False
        return True if any(want) else None
    hits = hit_list(mapper.query_draft(queries[0]))
    ohits, det = osk.query_draft(queries[0], threads=8, details=True)
    om = det["mappings"]
    omm = sorted(zip(om["qseq"].tolist(), om["rseq"].tolist(), om["rstart"].tolist(), om["sketch"].tolist(), om["shared"].tolist()))
    gm = mappings(mapper)
    if not (ok and hits == ohits and gm == omm):
        print(f"MISMATCH kmers case {case} seed {seed} k {k} w {w} fragment {frag}: hits {hits} vs {ohits}; mappings gpu {len(gm)} oracle {len(omm)}")
        sg, so = set(gm), set(omm)
        print("   only gpu", sorted(sg - so)[:4], "only oracle", sorted(so - sg)[:4])
        return False
    return True if ohits else None

for case in range(cases):
    if time_box and time.time() - t0 > time_box:
        break
    done = case + 1
    if history:
        with warnings.catch_warnings(), tempfile.TemporaryDirectory() as tmp:
            warnings.simplefilter("ignore")
            bad += 0 if history_case(g, case, tmp) else 1
        continue
    if contig_mode:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = contigs_case(g, case)
        degenerate += res is None
        bad += res is False
        continue
    if kmer_mode:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = kmers_case(g, case)
        degenerate += res is None
        bad += res is False
        continue
    if case % 10 == 9:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            bad += 0 if protein_case(g, case) else 1
        continue
    k = int(g.choice([8, 11, 12, 14, 16, 16, 16, 17, 21, 24]))
    frag = int(g.choice([200, 500, 1000, 1500, 3000, 3000, 5000]))
    pid = float(g.choice([70, 75, 80, 80, 85, 90, 95]))
    minfrac = float(g.choice([0.0, 0.1, 0.2, 0.5]))
    if default_cell:
        k, frag, pid = 16, 3000, 80.0
    params = dict(k=k, fragment_length=frag, percentage_identity=pid, minimum_fraction=minfrac)
    if domain:
        params["k"] = int(g.integers(5, 34))
        params["percentage_identity"] = float(g.choice([64.5, 65, 66, 67, 68, 69, 70, 96, 97, 98, 99, 99.5, 100]))
        params["p_value"] = float(10.0 ** -g.uniform(1, 12))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        osk = OracleSketch(**params)
        if osk.window_size >= frag:      # degenerate cell: nothing maps; covered by the unit tests
            degenerate += 1
            continue
        sk = pf.Sketch(**params, rules=RULES)
        # a third of the cases index with a narrow low word of the global coordinate (FA_GPOS_BITS, read when the index is built):
        # dozens of word boundaries inside these small indexes, i.e. the 64-bit form of k_l1's candidate scan
        os.environ.pop("FA_GPOS_BITS", None)
        if g.random() < 0.33:
            os.environ["FA_GPOS_BITS"] = str(max(12, int(2 * frag).bit_length() + 1) + int(g.integers(0, 3)))
        length = int(g.integers(max(3 * frag, 8000), 60_000))
        anc = scramble(g, syn.random_codes(g, length))
        n_ref = int(g.integers(1, 6))
        for i in range(n_ref):
            d = float(g.choice([0.0, 0.01, 0.03, 0.06, 0.1, 0.15]))
            r = scramble(g, syn.mutate_codes(g, anc, d)) if g.random() < 0.5 else syn.mutate_codes(g, anc, d)
            contigs = [to_bytes(g, x) for x in syn.split_contigs(g, r, int(g.integers(1, 5)))]
            if g.random() < 0.3: contigs.append(b"ACGT" * int(g.integers(0, 4)))
            sk.add_draft(i, contigs); osk.add_draft(i, contigs)
        if g.random() < 0.5:
            r = to_bytes(g, syn.random_codes(g, length)); sk.add_draft(n_ref, [r]); osk.add_draft(n_ref, [r])
        mapper = sk.index(); osk.index()
        queries = []
        for _ in range(int(g.integers(1, 4)) if case % 4 == 0 else 1):
            q = scramble(g, syn.mutate_codes(g, anc, float(g.choice([0.0, 0.02, 0.05, 0.1])))) if g.random() < 0.5 else syn.mutate_codes(g, anc, 0.03)
            plain = default_cell and g.random() < 0.6          # (default-cell runs: 60 % plain-ACGT queries, the rest with N runs / IUPAC / lower case)
            queries.append([(bytes(syn.to_ascii(x)) if plain else to_bytes(g, x)) for x in syn.split_contigs(g, q, int(g.integers(1, 4)))])
        if len(queries) > 1:
            # the resident-batch API must give, per genome, what one query_draft call gives
            got = [[(h.name, h.identity, h.matches, h.fragments) for h in hs] for hs in mapper.upload_genomes(queries).query()]
            want = [osk.query_draft(q, threads=8) for q in queries]
            if got != want:
                bad += 1
                print(f"MISMATCH batch case {case} seed {seed} params {params}: {got} vs {want}")
            continue
        query = queries[0]
        hits = [(h.name, h.identity, h.matches, h.fragments) for h in mapper.query_draft(query)]
        ohits, det = osk.query_draft(query, threads=8, details=True)
    om = det["mappings"]
    omm = sorted(zip(om["qseq"].tolist(), om["rseq"].tolist(), om["rstart"].tolist(), om["sketch"].tolist(), om["shared"].tolist()))
    try:
        gm = mappings(mapper)
    except (RuntimeError, NotImplementedError) as e:   # FA_PASS_FRAGMENTS: more parts than the stage getters retain
        if "stage getters" not in str(e):
            raise
        gm = omm
    ok = hits == ohits and gm == omm and len(mapper.lookup_index) == osk.index_size and mapper.occurences_threshold == osk.freq_threshold
    if not ok:
        bad += 1
        print(f"MISMATCH case {case} seed {seed} params {params} window {osk.window_size}: hits {hits} vs {ohits}; mappings gpu {len(gm)} oracle {len(omm)}")
        sg, so = set(gm), set(omm)
        print("   only gpu", sorted(sg - so)[:4], "only oracle", sorted(so - sg)[:4])
print(f"{done} {'history ' if history else ''}cases (seed {seed}{', ' + repr(RULES) if RULES else ''}), {bad} mismatches, {degenerate} degenerate, {time.time() - t0:.1f} s")
sys.exit(1 if bad else 0)
