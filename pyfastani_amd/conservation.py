"""What a mapping table is read for, computed where the records already are: per query fragment, how many relatives share it
and how well (``fa_mappings_profile``), and per genome the split into core and accessory fragments at any number of presence
thresholds (``fa_profile_summary``; include/fastani_hip.h has the semantics).  The records never leave HBM:
`GenomeBatch.iter_mappings_device` leaves every range's records in one device buffer and `FragmentProfile.add` reduces them
there, pass by pass, so an all-vs-all of any size comes down to 16 bytes per query fragment.

One caveat is part of the semantics.  The records are the mappings computeCGI KEPT: the best of a query fragment per
reference genome, then the best per reference bin.  A fragment that lost its reference bin to a neighbour is absent from that
reference's records, so ``count`` is "references whose hit counts this fragment", not "references where it would map".  The
same (query, fragment, reference) in two records is not detected and counts twice; the mapper never emits that.

The same records are reduced by reference position too (``fa_mappings_reference_profile``, `ReferenceProfile`): one entry per
reference bin, the key space the mapper keeps one mapping per (query genome, reference genome) for (`Mapper.reference_bins`).
The mapper emits at most one record per (query, reference genome, bin), so ``count[bin]`` is the number of query genomes whose
hit counts a mapping that STARTS in that bin.  Three properties of FastANI's binning follow.  Bins are 20 bases shorter than
fragments: with identical coordinates about one bin in ``fragment_length / 20`` holds no fragment start.  A start can slip
across a bin boundary: an indel moves a mapping's start a few bases into the neighbouring bin, which then holds two candidates
and keeps one, and the bin beside it stays empty for that query.  The last bin of a contig never receives a start, because no
whole fragment fits there.  One empty bin is therefore no evidence of absence; a run of two or more is, which is what
``min_length`` of the regions is for.  Both profiles are read as intervals -- core blocks, accessory islands --:
``fa_profile_regions`` (`ReferenceProfile.regions`, `FragmentProfile.regions`) returns the maximal runs of entries at or
above, or below, a presence threshold, per contig, in order.

There is no CPU path: without a HIP device the calls raise ``RuntimeError``, like every compute entry point.  Not imported by
the package itself (like `clusters`): it needs numpy and torch.
"""
import collections
import ctypes as C
import fractions

import numpy as np
import torch

from ._batch import MAPPING_DTYPE, REGION_DTYPE, ROW_DTYPE
from ._lib import check, lib

Summary = collections.namedtuple("Summary", "fragments hits sum")

STATS = ("counted", "skipped", "below", "on_chip_workgroups")


def _host_i32(values, n, what):
    """``values`` as a contiguous int32 array of ``n`` entries on the host, or None"""
    if values is None:
        return None
    values = np.ascontiguousarray(values.cpu().numpy() if hasattr(values, "cpu") else values)
    if values.shape != (n,) or values.dtype.kind not in "iu":
        raise ValueError(f"{what} holds one integer for each of the {n}")
    return values.astype(np.int32)


def _ptr(array):
    return C.c_void_p(array.ctypes.data) if array is not None else None


def _device(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _records(mappings, device):
    """``(keep-alive, n, address, on_device)`` of the records either profile's ``add`` takes"""
    if isinstance(mappings, np.ndarray):
        records = np.ascontiguousarray(mappings, dtype=MAPPING_DTYPE)
        return records, int(records.shape[0]), records.ctypes.data, 0
    if mappings.dtype != torch.int32 or mappings.dim() != 2 or mappings.shape[1] != 8 or mappings.device != device:
        raise ValueError("device mappings are an int32 [n, 8] tensor on the profile's device")
    records = mappings.contiguous()
    return records, int(records.shape[0]), records.data_ptr(), 1


def _summary(count, sum, n, offsets, min_count, device):
    """`fa_profile_summary` over ``n`` genomes whose entries ``offsets`` delimits"""
    need = np.ascontiguousarray(min_count.cpu().numpy() if hasattr(min_count, "cpu") else min_count)
    if need.dtype.kind not in "iu" or need.ndim not in (1, 2) or need.shape[-1] != n or (need.ndim == 2 and need.shape[0] < 1):
        raise ValueError("min_count is int [n_genomes], or [c, n_genomes] with c >= 1")
    if need.size and (int(need.min()) < 0 or int(need.max()) > np.iinfo(np.int32).max):
        raise ValueError("min_count must not be negative")
    need = need.astype(np.int32)
    n_sets = need.shape[0] if need.ndim == 2 else 1
    out = [torch.zeros(need.shape, dtype=torch.int64, device=device) for _ in range(3)]
    with torch.cuda.device(device):
        torch.cuda.synchronize(device)
        check(lib.fa_profile_summary(C.c_void_p(count.data_ptr()), C.c_void_p(sum.data_ptr()), n, _ptr(offsets), _ptr(need), n_sets,
                                     *[C.c_void_p(x.data_ptr()) for x in out], 1))
    return Summary(*out)


def _mean(count, sum):
    mean = sum.to(torch.float64) / count.clamp(min=1).to(torch.float64) / 2.0 ** 20
    return torch.where(count == 0, torch.full_like(mean, float("nan")), mean)


def _share(entries, offsets, device):
    """``entries`` per genome over the genome's number of entries, float64; NaN for a genome without entries"""
    total = torch.from_numpy(np.diff(offsets)).to(device)
    share = entries.to(torch.float64) / total.clamp(min=1).to(torch.float64)
    return torch.where(total == 0, torch.full_like(share, float("nan")), share)


def _regions(count, sum, offsets, need, below, min_length, device):
    """`fa_profile_regions` over the segments ``offsets`` delimits: a ``REGION_DTYPE`` array on the host"""
    if int(min_length) < 1:
        raise ValueError("min_length must be at least 1")
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = C.c_int64(0)
    args = (C.c_void_p(count.data_ptr()), C.c_void_p(sum.data_ptr()), len(need), _ptr(offsets), _ptr(need), 1 if below else 0, int(min_length))
    with torch.cuda.device(device):
        torch.cuda.synchronize(device)
        check(lib.fa_profile_regions(*args, None, 0, C.byref(n), 0))
        out = np.zeros(n.value, dtype=REGION_DTYPE)
        if n.value:
            check(lib.fa_profile_regions(*args, _ptr(out), n.value, C.byref(n), 0))
    return out


def _need_per_genome(need, n, what):
    need = np.asarray(need.cpu().numpy() if hasattr(need, "cpu") else need)
    if need.ndim == 0:
        need = np.full(n, need)
    if need.shape != (n,) or need.dtype.kind not in "iu" or (need.size and (int(need.min()) < 0 or int(need.max()) > np.iinfo(np.int32).max)):
        raise ValueError(f"need is one int, not negative, or one for each of the {n} {what}")
    return need.astype(np.int32)


class FragmentProfile:
    """The conservation profile of a batch of query genomes: ``count`` (int32), ``sum`` (int64, identities in fixed point,
    ``rint(identity * 2**20)``) and ``lowest`` (float32, ``+inf`` while nothing is counted), three tensors on ``device`` with
    one entry per query fragment.  Fragment ``f`` (``query_seq_id``, numbered as `outputs.fragment_coordinates` numbers it) of
    query ``q`` is entry ``fragment_offsets[q] + f``; ``fragment_counts`` is the batch's ``total_fragments``."""

    def __init__(self, fragment_counts, n_references, device="cuda"):
        counts = np.asarray(fragment_counts).astype(np.int64)
        if counts.ndim != 1 or (counts < 0).any():
            raise ValueError("fragment_counts holds one number of fragments, not negative, per query genome")
        if int(n_references) < 0:
            raise ValueError("n_references must not be negative")
        self.n_queries, self.n_references = len(counts), int(n_references)
        self.fragment_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.device = _device(device)
        total = int(self.fragment_offsets[-1])
        self.count = torch.zeros(total, dtype=torch.int32, device=self.device)
        self.sum = torch.zeros(total, dtype=torch.int64, device=self.device)
        self.lowest = torch.full((total,), float("inf"), dtype=torch.float32, device=self.device)

    def add(self, mappings, query_labels=None, reference_labels=None, self_reference=None, min_identity=0.0, stats=None):
        """Accumulates records: a ``MAPPING_DTYPE`` array on the host, or an int32 ``[n, 8]`` tensor of their words on the
        profile's device (what `GenomeBatch.iter_mappings_device` yields).  A record is counted iff its identity is at least
        ``min_identity`` (float32; equality counts), and, with labels, ``query_labels[query_id] ==
        reference_labels[ref_genome_id]`` -- both arrays or neither --, and, with ``self_reference``,
        ``self_reference[query_id] != ref_genome_id``: the reference that is the query itself, ``-1`` for none.  The result
        does not depend on the order of the records or on how they are split over calls.  ``stats``, a dict, receives
        ``counted``, ``skipped`` (by labels or self), ``below`` (``min_identity``) and ``on_chip_workgroups``.  An id out of
        range, or an identity that is NaN, negative (``-0.0`` included) or above 128, raises ``ValueError`` and leaves the
        profile as it was.  Returns the profile."""
        if (query_labels is None) != (reference_labels is None):
            raise ValueError("query_labels and reference_labels go together")
        ql = _host_i32(query_labels, self.n_queries, "query_labels")
        rl = _host_i32(reference_labels, self.n_references, "reference_labels")
        sr = _host_i32(self_reference, self.n_queries, "self_reference")
        records, n, ptr, on_device = _records(mappings, self.device)
        counters = (C.c_int64 * 4)()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)          # the library runs on a stream of its own: torch's writes are done
            check(lib.fa_mappings_profile(C.c_void_p(ptr), n, on_device, self.n_queries, _ptr(self.fragment_offsets), self.n_references,
                                          _ptr(ql), _ptr(rl), _ptr(sr), float(min_identity), C.c_void_p(self.count.data_ptr()),
                                          C.c_void_p(self.sum.data_ptr()), C.c_void_p(self.lowest.data_ptr()), counters))
        if stats is not None:
            for name, value in zip(STATS, counters):
                stats[name] = stats.get(name, 0) + int(value)
        return self

    def mean(self):
        """The mean identity of every fragment's counted records, float64 ``sum / count / 2**20``; NaN where ``count == 0``"""
        return _mean(self.count, self.sum)

    def summary(self, min_count):
        """Per genome, over its fragments with ``count >= min_count``: ``Summary(fragments, hits, sum)`` -- how many there
        are, the sum of their counts, the sum of their fixed-point sums --, int64 tensors on the profile's device of the
        shape of ``min_count``: int ``[n_queries]`` (`min_count_for`), or ``[c, n_queries]`` for ``c`` thresholds served by one
        walk of the fragments -- the presence curve.  The mean identity of a genome's core is ``sum / hits / 2**20``.  A
        genome without fragments gives zeros.  A negative ``min_count`` raises ``ValueError``."""
        return _summary(self.count, self.sum, self.n_queries, self.fragment_offsets, min_count, self.device)

    def core_fraction(self, min_count):
        """The share of every genome's fragments with ``count >= min_count``, float64 of the shape of ``min_count``; NaN for
        a genome without fragments"""
        return _share(self.summary(min_count).fragments, self.fragment_offsets, self.device)

    def regions(self, contig_lengths, fragment_length, need, below=False, min_length=1):
        """The maximal runs of fragments with ``count >= need`` (``below=True``: ``count < need``) inside one contig, as a
        ``REGION_DTYPE`` array in (segment, first) order; runs of fewer than ``min_length`` fragments are dropped.
        ``contig_lengths`` holds one sequence of contig lengths per genome, as `outputs.fragment_coordinates` takes them: the
        segments are the contigs of every genome, numbered through, a contig too short to hold a fragment an empty one.
        ``need`` is one int, or one per genome.  A region's ``first`` counts fragments from its contig's start: it covers
        bases ``[first * fragment_length, (first + length) * fragment_length)`` (`outputs.write_regions`)."""
        if int(fragment_length) < 1:
            raise ValueError("fragment_length must be positive")
        if len(contig_lengths) != self.n_queries:
            raise ValueError("one sequence of contig lengths per query genome")
        per_contig = [np.asarray(lengths, dtype=np.int64).reshape(-1) // int(fragment_length) for lengths in contig_lengths]
        if [int(c.sum()) for c in per_contig] != np.diff(self.fragment_offsets).tolist():
            raise ValueError("the contig lengths do not give the profile's number of fragments per genome")
        need = _need_per_genome(need, self.n_queries, "genomes")
        offsets = np.concatenate([[0], np.cumsum(np.concatenate(per_contig + [np.zeros(0, np.int64)]))]).astype(np.int64)
        per_segment = np.repeat(need, [len(c) for c in per_contig]).astype(np.int32)
        return _regions(self.count, self.sum, offsets, per_segment, below, min_length, self.device)


class ReferenceProfile:
    """The conservation profile of the references of a mapper: ``count`` (int32), ``sum`` (int64, identities in fixed point)
    and ``lowest`` (float32, ``+inf`` while nothing is counted), three tensors on ``device`` with one entry per reference bin.
    ``mapper_or_bins`` is a `Mapper`, or the tuple `Mapper.reference_bins` returns; ``bin_length``, ``contig_bin`` and
    ``contig_genome`` are that tuple, ``genome_bin`` [n_references + 1] the first bin of every reference genome.  A mapping
    on contig ``c`` at ``ref_start_pos`` is entry ``contig_bin[c] + ref_start_pos // bin_length``.  ``count[bin]`` is the
    number of query genomes whose hit counts a mapping that starts in the bin: one empty bin is no evidence of absence (the
    module docstring has the three reasons), a run of two or more is."""

    def __init__(self, mapper_or_bins, n_queries, device=None, n_references=None):
        if hasattr(mapper_or_bins, "reference_bins"):
            bins = mapper_or_bins.reference_bins()
            n_references = len(mapper_or_bins.names) if n_references is None else n_references
            device = mapper_or_bins._torch_device() if device is None else device
        else:
            bins = mapper_or_bins
        bin_length, contig_bin, contig_genome = bins
        self.bin_length = int(bin_length)
        self.contig_bin = np.ascontiguousarray(contig_bin, dtype=np.int32)
        self.contig_genome = np.ascontiguousarray(contig_genome, dtype=np.int32)
        if self.bin_length < 1 or self.contig_bin.ndim != 1 or self.contig_genome.shape != (len(self.contig_bin) - 1,):
            raise ValueError("bins are (bin_length >= 1, contig_bin [n_contigs + 1], contig_genome [n_contigs])")
        if self.contig_bin[0] != 0 or (np.diff(self.contig_bin) < 0).any():
            raise ValueError("contig_bin starts at 0 and does not decrease")
        if int(n_queries) < 0:
            raise ValueError("n_queries must not be negative")
        if n_references is None:
            n_references = int(self.contig_genome[-1]) + 1 if len(self.contig_genome) else 0
        self.n_queries, self.n_references, self.n_contigs = int(n_queries), int(n_references), len(self.contig_genome)
        if len(self.contig_genome) and ((np.diff(self.contig_genome) < 0).any() or self.contig_genome[0] < 0 or
                                        self.contig_genome[-1] >= self.n_references):
            raise ValueError("contig_genome does not decrease and stays inside [0, n_references)")
        first_contig = np.searchsorted(self.contig_genome, np.arange(self.n_references + 1))
        self.genome_bin = self.contig_bin[first_contig].astype(np.int64)
        self.device = _device("cuda" if device is None else device)
        total = int(self.contig_bin[-1])
        self.count = torch.zeros(total, dtype=torch.int32, device=self.device)
        self.sum = torch.zeros(total, dtype=torch.int64, device=self.device)
        self.lowest = torch.full((total,), float("inf"), dtype=torch.float32, device=self.device)

    def add(self, mappings, query_labels=None, reference_labels=None, self_reference=None, min_identity=0.0, stats=None):
        """Accumulates records, in the forms and under the filters of `FragmentProfile.add`: a ``MAPPING_DTYPE`` array on the
        host, or an int32 ``[n, 8]`` tensor on the profile's device.  ``stats`` receives ``counted``, ``skipped`` and
        ``below``.  An id out of range, a contig of another reference genome, a position outside the bins of its contig, or
        an identity that is NaN, negative or above 128 raises ``ValueError`` and leaves the profile as it was.  Returns the
        profile."""
        if (query_labels is None) != (reference_labels is None):
            raise ValueError("query_labels and reference_labels go together")
        ql = _host_i32(query_labels, self.n_queries, "query_labels")
        rl = _host_i32(reference_labels, self.n_references, "reference_labels")
        sr = _host_i32(self_reference, self.n_queries, "self_reference")
        records, n, ptr, on_device = _records(mappings, self.device)
        counters = (C.c_int64 * 3)()
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)          # the library runs on a stream of its own: torch's writes are done
            check(lib.fa_mappings_reference_profile(C.c_void_p(ptr), n, on_device, self.n_queries, self.n_references, self.n_contigs,
                                                    _ptr(self.contig_bin), _ptr(self.contig_genome), self.bin_length, _ptr(ql), _ptr(rl),
                                                    _ptr(sr), float(min_identity), C.c_void_p(self.count.data_ptr()),
                                                    C.c_void_p(self.sum.data_ptr()), C.c_void_p(self.lowest.data_ptr()), counters))
        if stats is not None:
            for name, value in zip(STATS, counters):
                stats[name] = stats.get(name, 0) + int(value)
        return self

    def mean(self):
        """The mean identity of every bin's counted records, float64 ``sum / count / 2**20``; NaN where ``count == 0``"""
        return _mean(self.count, self.sum)

    def summary(self, min_count):
        """Per REFERENCE genome, over its bins with ``count >= min_count``: ``Summary(fragments, hits, sum)`` -- ``fragments``
        is the number of such bins -- as `FragmentProfile.summary` gives it; ``min_count`` is int ``[n_references]`` or
        ``[c, n_references]``."""
        return _summary(self.count, self.sum, self.n_references, self.genome_bin, min_count, self.device)

    def covered_fraction(self, min_count):
        """The share of every reference genome's bins with ``count >= min_count``, float64 of the shape of ``min_count``;
        NaN for a genome without bins.  The bins that can never hold a start -- the last of every contig, about one in
        ``fragment_length / 20`` of the others -- count as uncovered."""
        return _share(self.summary(min_count).fragments, self.genome_bin, self.device)

    def regions(self, need, below=False, min_length=1):
        """The maximal runs of bins with ``count >= need`` (``below=True``: ``count < need``) inside one contig, as a
        ``REGION_DTYPE`` array in (segment, first) order: ``segment`` is the contig (``ref_seq_id``), ``first`` the run's first
        bin counted from the contig's start.  ``need`` is one int, or one per reference genome.  Runs of fewer than
        ``min_length`` bins are dropped: ask for 2 when looking for absence, since one empty bin is none."""
        need = _need_per_genome(need, self.n_references, "reference genomes")
        per_contig = need[self.contig_genome] if self.n_contigs else np.zeros(0, np.int32)
        return _regions(self.count, self.sum, self.contig_bin.astype(np.int64), np.ascontiguousarray(per_contig, dtype=np.int32), below,
                        min_length, self.device)


def _rational(share):
    """A share as a `fractions.Fraction`: a Fraction or an int as it is, ``(numerator, denominator)``, or a float or a
    string read as the decimal number it prints as (0.9 is 9/10, not the binary fraction next to it)"""
    if isinstance(share, tuple):
        share = fractions.Fraction(int(share[0]), int(share[1]))
    elif isinstance(share, (float, np.floating)):
        share = fractions.Fraction(repr(float(share)))
    else:
        share = fractions.Fraction(share)
    if not 0 <= share <= 1:
        raise ValueError("a share lies in [0, 1]")
    return share


def min_count_for(labels, share):
    """The ``min_count`` of "present in at least ``share`` of the other members of its cluster": per genome
    ``ceil(share * (cluster size - 1))``, int32 ``[n]``, for a partition ``labels`` as `clusters.clusters` returns it (numpy
    or a tensor).  ``share`` is rational -- a `fractions.Fraction`, ``(numerator, denominator)``, or a float or string read
    as the decimal number it prints as -- and the ceiling is taken in integers, never through a float product."""
    labels = np.ascontiguousarray(labels.cpu().numpy() if hasattr(labels, "cpu") else labels)
    if labels.ndim != 1 or labels.dtype.kind not in "iu":
        raise ValueError("labels holds one cluster label per genome")
    share = _rational(share)
    _, inverse, sizes = np.unique(labels, return_inverse=True, return_counts=True)
    others = [int(s) - 1 for s in sizes]
    need = np.array([-((-share.numerator * m) // share.denominator) for m in others], dtype=np.int64)
    return need[inverse.reshape(-1)].astype(np.int32)


def all_vs_all(mapper, batch, labels=None, self_reference=None, min_identity=0.0, stats=None):
    """The profile of a resident batch mapped against the mapper's references, range by range
    (`GenomeBatch.iter_mappings_device` and `FragmentProfile.add`): returns ``(profile, rows)``, the filled `FragmentProfile`
    and the ``ROW_DTYPE`` rows of the whole batch.  ``labels`` is one array over the genomes when the batch IS the reference
    set, or ``(query_labels, reference_labels)``; ``self_reference[q]`` is the reference that is query ``q`` itself
    (``numpy.arange(n)`` for one set mapped against itself), ``-1`` for none."""
    if labels is None:
        query_labels = reference_labels = None
    elif isinstance(labels, tuple):
        query_labels, reference_labels = labels
    else:
        query_labels = reference_labels = labels
    profile = FragmentProfile(batch.total_fragments, len(mapper.names), device=mapper._torch_device())
    rows = []
    for _, _, range_rows, maps in batch.iter_mappings_device():
        profile.add(maps, query_labels, reference_labels, self_reference, min_identity, stats)
        rows.append(range_rows)
    return profile, (np.concatenate(rows) if rows else np.zeros(0, dtype=ROW_DTYPE))


def reference_all_vs_all(mapper, batch, labels=None, self_reference=None, min_identity=0.0, stats=None, fragment_profile=None):
    """The reference-side profile of a resident batch mapped against the mapper's references, range by range: returns
    ``(reference_profile, rows)``, the filled `ReferenceProfile` and the ``ROW_DTYPE`` rows of the whole batch.  The arguments
    are those of `all_vs_all`.  With ``fragment_profile``, a `FragmentProfile` of the batch, the same device records feed it
    too, so that one mapping pass gives both profiles; ``stats`` counts the reference side."""
    if labels is None:
        query_labels = reference_labels = None
    elif isinstance(labels, tuple):
        query_labels, reference_labels = labels
    else:
        query_labels = reference_labels = labels
    profile = ReferenceProfile(mapper, len(batch.total_fragments))
    rows = []
    for _, _, range_rows, maps in batch.iter_mappings_device():
        profile.add(maps, query_labels, reference_labels, self_reference, min_identity, stats)
        if fragment_profile is not None:
            fragment_profile.add(maps, query_labels, reference_labels, self_reference, min_identity)
        rows.append(range_rows)
    return profile, (np.concatenate(rows) if rows else np.zeros(0, dtype=ROW_DTYPE))
