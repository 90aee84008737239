"""The bottom-s signatures of a resident query batch (fa_genomes_signatures, pyfastani_amd/csrc/fa_batchsig.hip.h), restated
with the CPU oracle and numpy, and the named cases both test files run.

  fragments   every contig of at least fragment_length, cut into its whole fragments
  sketch      OracleSketch.sketch_sequence of each fragment: the hashes of its winnowed minimizers
  signature   np.unique over a genome's fragments, cut at s

tests/test_batch_signatures_inputs.py checks the restatement on the CPU against a second definition (a sketch to which
every fragment was added as a contig of its own) and the cases against their purposes;
tests/test_gpu_batch_signatures.py compares the library with it byte for byte.
"""
import functools
import os

import numpy as np

from conftest import read_fasta
from oracle.oracle import OracleSketch
from pyfastani_amd import synthetic as syn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PROTEIN_FILES = ("BGC0001425.faa", "BGC0001427.faa", "BGC0001428.faa")

# the (k, w) cells the sketch kernel is built for with both parameters at compile time (fa_k1.hip.h); any other window of
# these k takes the run-time form
COMPILE_TIME_CELLS = {(14, 12), (14, 37), (14, 50), (16, 13), (16, 24), (16, 40), (21, 15), (21, 25)}

# name -> the keywords of Sketch / OracleSketch
PARAMETER_SETS = {
    "default": dict(k=16, fragment_length=3000),                   # w = 24: a compile-time cell
    "run_time_window": dict(k=16, fragment_length=2000),           # w = 16: the run-time form of k = 16
    "k21": dict(k=21, fragment_length=3000),                       # w = 15
    "fragment_500": dict(k=16, fragment_length=500),               # w = 6
    "protein": dict(protein=True, fragment_length=100),            # w = 1, k_sketch_tiles (what the protein tests use)
}

FIXED_SIZES = (1, 2, 63, 64, 65, 1000, 4096)
REPEATS = 40
SMALL_GENOMES = 40

# what the genomes of genome_set() are there for, by number; the small genomes follow "exceptions", and the last genome
# has no contig again
GENOMES = {"no_contig": 0, "short_contigs_only": 1, "one_fragment": 2, "around_the_fragment_length": 3, "repeated_fragment": 4,
           "exceptions": 5, "first_small": 6}


def _nucleotide_set(frag, seed):
    g = syn.rng(seed)

    def random(n):
        return syn.to_ascii(syn.random_codes(g, n)).tobytes().decode("ascii")
    unit = random(frag)
    plain = random(2 * frag)
    # an N run that spans several windows, and IUPAC codes one by one, all inside the first fragment; one more N in the second
    marked = list(plain)
    marked[frag // 3: frag // 3 + 50] = "N" * 50
    for at, code in ((frag // 2, "R"), (frag // 2 + 7, "Y"), (frag - 20, "K"), (frag + frag // 2, "N")):
        marked[at] = code
    genomes = [
        [],
        [random(frag - 1), random(100)],
        [random(frag)],
        [random(frag - 1), random(frag), random(2 * frag + 5)],
        [unit * REPEATS],
        ["".join(marked)],
    ]
    genomes += [[random(frag + (i % 3) * (frag // 2))] for i in range(SMALL_GENOMES)]          # one fragment each, some with a tail
    genomes.append([])
    return genomes


def _protein_set(frag):
    records = [r for name in PROTEIN_FILES for r in read_fasta(os.path.join(GOLDEN, name))]
    long_ones = [r for r in records if len(r) >= frag]
    assert len(long_ones) >= SMALL_GENOMES + 4, len(long_ones)
    by_length = sorted(long_ones, key=len)
    three = next(r for r in by_length if len(r) >= 2 * frag + 5)
    genomes = [
        [],
        [by_length[4][: frag - 1], by_length[5][: frag // 3]],         # (every golden record is longer than a fragment: two heads)
        [by_length[0][:frag]],
        [by_length[1][: frag - 1], by_length[2][:frag], three[: 2 * frag + 5]],
        [by_length[3][:frag] * REPEATS],
        [by_length[-1]],                                             # (proteins have no exception tiles: the longest record instead)
    ]
    genomes += [[r] for r in long_ones[:SMALL_GENOMES]]
    genomes.append([])
    return genomes


@functools.lru_cache(maxsize=None)
def genome_set(name):
    """the genomes of a parameter set: a list of genomes, each a list of contigs (str)"""
    params = PARAMETER_SETS[name]
    if params.get("protein"):
        return _protein_set(params["fragment_length"])
    return _nucleotide_set(params["fragment_length"], 7000 + sorted(PARAMETER_SETS).index(name))


def fragments_of(contigs, frag):
    """the whole fragments of every contig of at least a fragment, in order"""
    return [c[i * frag: (i + 1) * frag] for c in contigs if len(c) >= frag for i in range(len(c) // frag)]


def fragment_counts(name):
    frag = PARAMETER_SETS[name]["fragment_length"]
    return [len(fragments_of(contigs, frag)) for contigs in genome_set(name)]


# ---- the restatement -------------------------------------------------------------------------------------------------
def hash_sets_of(genomes, params):
    """every genome's distinct hashes, ascending (uint32): np.unique over the oracle's sketch of each of its fragments"""
    osk = OracleSketch(**params)
    out = []
    for contigs in genomes:
        sketches = [osk.sketch_sequence(f)[0] for f in fragments_of(contigs, params.get("fragment_length", 3000))]
        out.append(np.unique(np.concatenate(sketches)) if sketches else np.zeros(0, np.uint32))
    return out


@functools.lru_cache(maxsize=None)
def hash_sets(name):
    return hash_sets_of(genome_set(name), PARAMETER_SETS[name])


def cut(sets, s):
    """(sig uint32 [n, s], count int32 [n]) of ascending distinct hash arrays"""
    sig = np.zeros((len(sets), s), dtype=np.uint32)
    tally = np.zeros(len(sets), dtype=np.int32)
    for i, mine in enumerate(sets):
        mine = mine[:s]
        sig[i, : len(mine)], tally[i] = mine, len(mine)
    return sig, tally


def record_counts(name):
    """the minimizer records of every genome (duplicates and all)"""
    params = PARAMETER_SETS[name]
    osk = OracleSketch(**params)
    return [sum(len(osk.sketch_sequence(f)[0]) for f in fragments_of(contigs, params["fragment_length"])) for contigs in genome_set(name)]


def restate_signatures(name, s, first=0, count=None):
    """(sig uint32 [count, s], count int32 [count]) of the genomes [first, first + count)"""
    sets = hash_sets(name)
    count = len(sets) - first if count is None else count
    return cut(sets[first: first + count], s)


def sizes(name):
    """the signature sizes of a parameter set: the fixed ones, and d - 1, d, d + 1 around the distinct hashes of the
    repeated-fragment genome"""
    d = len(hash_sets(name)[GENOMES["repeated_fragment"]])
    return tuple(sorted(set(FIXED_SIZES) | {d - 1, d, d + 1}))


# ---- passes ----------------------------------------------------------------------------------------------------------
def pass_sizes(name, first=0, count=None):
    """0 (the library's own), 1, 2, 7, the fragments of the range, and more than that"""
    counts = fragment_counts(name)
    count = len(counts) - first if count is None else count
    total = sum(counts[first: first + count])
    return (0, 1, 2, 7, total, total + 5)


def pass_cuts(counts, size):
    """the fragment numbers at which passes of `size` fragments end, the last one included"""
    total = sum(counts)
    return list(range(size, total, size)) + ([total] if total else [])


def expected_stats(name, size, first=0, count=None, library_pass=48 * 1024):
    counts = fragment_counts(name)
    count = len(counts) - first if count is None else count
    total = sum(counts[first: first + count])
    size = size or library_pass
    return total, -(-total // size)
