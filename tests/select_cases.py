"""fa_sketch_select / fa_sketch_frequency (pyfastani_amd/csrc/fa_select.hip.h, pyfastani_amd.groups) restated in plain numpy,
and the named cases the three GPU test files and tests/test_select_inputs.py run.

  select      per selected genome: the records whose contig id lies in its contig range, contig ids shifted
  frequency   np.unique with counts, `sharding.frequency_threshold` over the counts, the keys at or above it

tests/test_select_inputs.py checks on the CPU, with the oracle's minimizers, that the restatement is the right definition and
that every case holds what it is there for; the GPU tests compare the library with it byte for byte.
"""
import functools

import numpy as np

from pyfastani_amd import sharding
from pyfastani_amd import synthetic as syn

import screen as sc

INT_MAX = 2**31 - 1
# k_select_copy (fa_select.hip.h): a workgroup of SEL_THREADS threads copies SEL_TILE = SEL_THREADS * SEL_PER_THREAD consecutive
# output records per trip, lane l of a wave taking record base + l; the sizes below are stated against these
WAVE, SEL_THREADS, SEL_PER_THREAD = 64, 256, 4
SEL_TILE = SEL_THREADS * SEL_PER_THREAD


# ---- the restatement -------------------------------------------------------------------------------------------------
def restate_select(hash, seq_id, wpos, lengths, sbf, genomes):
    """(hash', seq_id', wpos', lengths', sbf', counter') of the selection, the definition of include/fastani_hip.h"""
    out_h, out_s, out_w, out_len, out_sbf, contigs = [], [], [], [], [], 0
    for g in genomes:
        first, end = (int(sbf[g - 1]) if g else 0), int(sbf[g])
        mine = (seq_id >= first) & (seq_id < end)
        out_h.append(hash[mine])
        out_s.append(seq_id[mine] - first + contigs)
        out_w.append(wpos[mine])
        contigs += end - first
        out_len.append(lengths[g])
        out_sbf.append(contigs)
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)      # noqa: E731
    return (cat(out_h, np.uint32), cat(out_s, np.int32), cat(out_w, np.int32), np.array(out_len, dtype=np.uint64),
            np.array(out_sbf, dtype=np.int32), contigs)


def restate_frequency(hash):
    """(threshold, the distinct hashes with at least that many records, ascending uint32)"""
    keys, counts = np.unique(np.asarray(hash, dtype=np.uint32), return_counts=True)
    threshold = sharding.frequency_threshold(np.sort(counts)[::-1], len(keys))
    return threshold, (keys[counts >= threshold] if threshold < INT_MAX else keys[:0])


# ---- the collection of the select tests ------------------------------------------------------------------------------
# the genomes of awkward() by number: the twelve of tests/screen.py::family_genomes() are the numbers not named here
AWKWARD = {"no_contig": 2, "short_contigs_only": 5, "one_record": 7, "fewer_records_than_a_wave": 10, "draft": 12, "no_contig_last": 17}
AWKWARD_SEED = 4100                # (any seed does: tests/test_select_inputs.py says what the genomes have to give)
FAMILY_SLOTS = [g for g in range(18) if g not in AWKWARD.values()]


def window_size():
    from oracle.oracle import OracleSketch
    return OracleSketch().window_size


@functools.lru_cache(maxsize=None)
def awkward():
    """eighteen genomes, each a list of contigs (ASCII arrays)"""
    g = syn.rng(AWKWARD_SEED)
    k, w = 16, window_size()
    random = lambda n: syn.to_ascii(syn.random_codes(g, n))                                             # noqa: E731
    special = {
        "no_contig": [],
        "short_contigs_only": [random(w - 1), random(3), random(k - 1)],       # not one of them is admitted: contigs, no record
        "one_record": [random(k + w - 1)],                                     # one window
        "fewer_records_than_a_wave": [random(300), random(5), random(200)],
        "draft": syn.split_contigs(g, random(100_000), 40),
        "no_contig_last": [],
    }
    genomes = [None] * 18
    for name, at in AWKWARD.items():
        genomes[at] = special[name]
    for at, genome in zip(FAMILY_SLOTS, sc.family_genomes()):
        genomes[at] = [genome]
    return genomes


def awkward_names():
    return [f"genome{g}" for g in range(18)]


@functools.lru_cache(maxsize=None)
def selections():
    """name -> ascending genome numbers"""
    a = AWKWARD
    out = {"nothing": [], "everything": list(range(18)), "first_only": [0], "last_only": [17], "stride_of_three": list(range(0, 18, 3)),
           "genomes_without_records": [a["no_contig"], a["short_contigs_only"], a["no_contig_last"]],
           "segments_shorter_than_a_wave": [a["no_contig"], a["one_record"], a["fewer_records_than_a_wave"]],
           # a segment of several SEL_TILEs in front of, and behind, a segment of one record
           "several_tiles_then_one_record": [6, a["one_record"]], "one_record_then_several_tiles": [a["one_record"], 8],
           "draft_between_neighbours": [11, a["draft"], 13]}
    out.update({f"only_{g:02d}": [g] for g in range(18)})
    return out


# ---- the frequency case ----------------------------------------------------------------------------------------------
FREQUENCY_SEED = 53                # (chosen on the CPU: tests/test_select_inputs.py says what it has to give)
FREQUENCY_PARTITIONS = ([[0, 2, 4], [1, 3, 5]], [[0], [1, 2, 3, 4, 5]])


@functools.lru_cache(maxsize=None)
def frequency_case():
    """(references, queries), each a list of contig lists: six 1 Mb references; two planted 45-mers sit in genomes 0 AND 1,
    about 150 and 75 times each, so their hashes reach the threshold over the whole collection and whether a group ignores
    them on its own depends on which of the two genomes it holds"""
    g = syn.rng(FREQUENCY_SEED)
    n = 1_000_000
    genomes = [syn.random_codes(g, n) for _ in range(6)]
    r1, r2 = syn.random_codes(g, 45), syn.random_codes(g, 45)
    for m in genomes[:2]:
        for p in range(1000, n - 1000, n // 150):
            m[p: p + 45] = r1
        for p in range(2500, n - 1000, n // 75):
            m[p: p + 45] = r2
    refs = [[syn.to_ascii(x)] for x in genomes]
    queries = [[syn.to_ascii(syn.mutate_codes(g, genomes[0], 0.02))], [syn.to_ascii(syn.mutate_codes(g, genomes[3], 0.04))],
               [syn.to_ascii(syn.mutate_codes(g, genomes[1], 0.01))]]
    return refs, queries


# ---- the family case -------------------------------------------------------------------------------------------------
FAMILY_PARTITION = [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]


def family_genomes():
    """the twelve genomes of tests/screen.py as contig lists (FAMILY_SEED there was chosen on the CPU; tests/test_select_inputs.py
    adds what this file needs of them: rows off the diagonal in every family)"""
    return [[genome] for genome in sc.family_genomes()]


def same_family(rows):
    return rows[rows["query_id"] // 4 == rows["ref_genome_id"] // 4]
