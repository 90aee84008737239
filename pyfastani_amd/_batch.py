"""Row layout of the hit table (``cgi::CGI_Results``, include/fastani/cgi/cgid_types.pxd:19-27 of the reference, plus the
query index of a batch) as a numpy structured dtype, and the resident-batch class (implemented in the compiled binding)."""
import os

import numpy as np

from ._fastani import GenomeBatch  # noqa: F401  (re-export)

ROW_DTYPE = np.dtype(
    [("query_id", "<i4"), ("ref_genome_id", "<i4"), ("count_seq", "<i4"), ("total_query_fragments", "<i4"),
     ("identity", "<f4")]
)
assert ROW_DTYPE.itemsize == 20

# one mapping that computeCGI kept (``fa_hit_mapping``): what `GenomeBatch.query_mappings` and
# `Mapper.query_draft_mappings` return beside the rows
MAPPING_DTYPE = np.dtype(
    [("query_id", "<i4"), ("query_seq_id", "<i4"), ("ref_genome_id", "<i4"), ("ref_seq_id", "<i4"), ("ref_start_pos", "<i4"),
     ("sketch_size", "<i4"), ("conserved", "<i4"), ("identity", "<f4")]
)
assert MAPPING_DTYPE.itemsize == 32

# one unordered genome pair of an all-vs-all table (``fa_pair``): what `pyfastani_amd.clusters.pairs` returns.  ``a < b``;
# ``identity_ab`` is query a on reference b, NaN where that row is missing or filtered; ``identity`` the symmetric value
PAIR_DTYPE = np.dtype(
    [("a", "<i4"), ("b", "<i4"), ("identity_ab", "<f4"), ("identity_ba", "<f4"), ("identity", "<f8")]
)
assert PAIR_DTYPE.itemsize == 24

# one merge of an average-linkage dendrogram (``fa_merge``): what `pyfastani_amd.clusters.dendrogram` keeps.  The clusters
# labelled ``lo < hi`` (their smallest genomes), of ``size_lo`` and ``size_hi`` genomes, merge into ``lo``; ``s`` is the fixed-point
# sum of the identities over all ``size_lo * size_hi`` genome pairs between them, ``present`` of those pairs have a row
MERGE_DTYPE = np.dtype(
    [("lo", "<i4"), ("hi", "<i4"), ("size_lo", "<i4"), ("size_hi", "<i4"), ("s", "<i8"), ("present", "<i8")]
)
assert MERGE_DTYPE.itemsize == 32

# one region of a conservation profile (``fa_profile_region``): what `conservation.ReferenceProfile.regions` and
# `conservation.FragmentProfile.regions` return.  A maximal run of ``length`` entries of contig ``segment`` from its entry
# ``first`` on; ``hits`` is the sum of their counts, ``sum`` that of their fixed-point identity sums
REGION_DTYPE = np.dtype(
    [("segment", "<i4"), ("first", "<i4"), ("length", "<i4"), ("reserved", "<i4"), ("hits", "<i8"), ("sum", "<i8")]
)
assert REGION_DTYPE.itemsize == 32


def pass_fragments():
    """Fragments the library maps per pass (``FA_PASS_FRAGMENTS``; 49152 by default, as in ``csrc/fa_knobs.h``).  The library
    reads the variable once, at its first pass; this reads it on every call, so set it before the first query."""
    return int(os.environ.get("FA_PASS_FRAGMENTS") or 48 * 1024)


def plan_ranges(fragment_counts, pass_fragments, first=0, count=None):
    """Genomes [first, first + count) cut into consecutive ranges ``[(first_genome, n_genomes), ...]`` the way the library
    cuts a call into passes: a range takes genomes while their fragments stay within ``pass_fragments``, and always at least
    one, so a single larger genome is a range of its own.  Every genome of the range is in exactly one of them, in order."""
    counts = [int(x) for x in fragment_counts]
    count = len(counts) - first if count is None else count
    if first < 0 or count < 0 or first + count > len(counts):
        raise ValueError("genome range out of bounds")
    if pass_fragments < 1:
        raise ValueError("pass_fragments must be positive")
    out, g0, end = [], first, first + count
    while g0 < end:
        g1, total = g0 + 1, counts[g0]
        while g1 < end and total + counts[g1] <= pass_fragments:
            total += counts[g1]
            g1 += 1
        out.append((g0, g1 - g0))
        g0 = g1
    return out
