"""The genomes of test_ingest_roads_host.py and test_gpu_ingest_roads.py: contigs that sit on the lengths where an ingest
rule turns (zero, the admission rule of the sketch, whole fragments), a genome without contigs and one with short contigs
only, and the roads by which Python hands them to the library as references."""
import warnings

import numpy as np

import pyfastani_amd as pf

RESIDUES = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
NAMES = ["edge_lo", "edge_hi", "edge_frag", "one_contig", "no_contigs", "short_only"]


def contig_lengths(sk):
    """Per genome, the contig lengths: four genomes on the edges, one without contigs, one with short contigs only."""
    k, w, frag = sk.k, sk.window_size, sk.fragment_length
    lo, hi = min(w, k), max(w, k)
    return [[0, lo - 1, lo, 3 * frag + 17], [hi - 1, hi, frag - 1, 12 * frag + 3], [frag, frag + 1, 2 * frag - 1, 20 * frag + 1],
            [17 * frag + 100], [], [lo - 1, 0]]


def make_genomes(sk, seed=20260):
    """The genomes as lists of `bytes` contigs: consecutive pieces of copies of one ancestor, two to five percent of
    substitutions each, so that every genome with fragments maps onto the others."""
    g = np.random.Generator(np.random.PCG64(seed))
    letters = RESIDUES if sk.protein else np.frombuffer(b"ACGT", np.uint8)
    lengths = contig_lengths(sk)
    anc = g.integers(0, len(letters), max(sum(ls) for ls in lengths), dtype=np.uint8)
    genomes = []
    for gi, ls in enumerate(lengths):
        codes = anc.copy()
        hit = g.random(len(codes)) < 0.02 + 0.01 * gi
        codes[hit] = (codes[hit] + g.integers(1, len(letters), int(hit.sum()), dtype=np.uint8)) % len(letters)
        seq, at, contigs = letters[codes].tobytes(), 0, []
        for n in ls:
            contigs.append(seq[at:at + n])
            at += n
        genomes.append(contigs)
    return genomes


def write_fastas(tmp_path, genomes):
    """One file per genome, lines of 70; a contig of length zero is a header without lines, a genome without contigs an empty file."""
    paths = []
    for gi, contigs in enumerate(genomes):
        path = tmp_path / f"{NAMES[gi]}.fa"
        with open(path, "wb") as f:
            for ci, c in enumerate(contigs):
                f.write(b">c%d of %d\n" % (ci, gi))
                for j in range(0, len(c), 70):
                    f.write(c[j:j + 70] + b"\n")
        paths.append(str(path))
    return paths


def expected_state(sk, genomes):
    """What Sketch._add_draft leaves (_fastani.pyx:610-690), restated: lengths, sequencesByFileInfo, counter, and the
    short-contig warnings per genome."""
    k, w, frag = sk.k, sk.window_size, sk.fragment_length
    lengths, by_file, shorts, counter = [], [], [], 0
    for contigs in genomes:
        lengths.append(sum(len(c) // frag * frag for c in contigs))
        shorts.append(sum(1 for c in contigs if len(c) < w or len(c) < k))
        counter += len(contigs)
        by_file.append(counter)
    return (lengths, by_file, counter), shorts


# every road Python offers for reference genomes: road(sketch, genomes, paths) -> warnings per call
def _calls(fns):
    counts = []
    for fn in fns:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
        assert all(issubclass(c.category, UserWarning) and "short contig" in str(c.message) for c in caught)
        counts.append(len(caught))
    return counts


def road_add_draft(sk, genomes, paths):
    return _calls([(lambda i=i: sk.add_genome(NAMES[i], genomes[i][0]) if len(genomes[i]) == 1 else sk.add_draft(NAMES[i], genomes[i]))
                   for i in range(len(genomes))])


def road_add_drafts(sk, genomes, paths):
    return _calls([lambda: sk.add_drafts(NAMES, genomes)])


def road_add_fasta(sk, genomes, paths):
    return _calls([(lambda i=i: sk.add_fasta(NAMES[i], paths[i])) for i in range(len(paths))])


def road_add_fasta_many(sk, genomes, paths):
    return _calls([lambda: sk.add_fasta_many(NAMES, paths)])


def road_add_packed(sk, genomes, paths):
    packed = pf.PackedGenomes(paths, protein=sk.protein)
    return _calls([lambda: sk.add_packed(NAMES[:4], packed, 0, 4), lambda: sk.add_packed(NAMES[4:], packed, 4)])


def road_add_fasta_stream(sk, genomes, paths):
    return _calls([lambda: sk.add_fasta_stream(NAMES, paths, chunk=2)])


def road_add_fasta_stream_keep(sk, genomes, paths):
    keep = pf.PackedGenomes([], protein=sk.protein)
    counts = _calls([lambda: sk.add_fasta_stream(NAMES, paths, chunk=2, keep=keep)])
    assert keep.paths == paths
    return counts


ROADS = [road_add_draft, road_add_drafts, road_add_fasta, road_add_fasta_many, road_add_packed, road_add_fasta_stream,
         road_add_fasta_stream_keep]
