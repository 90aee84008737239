"""What a mapping table is read for, computed where the records already are: per query fragment, how many relatives share it
and how well (``fa_mappings_profile``), and per genome the split into core and accessory fragments at any number of presence
thresholds (``fa_profile_summary``; include/fastani_hip.h has the semantics).  The records never leave HBM:
`GenomeBatch.iter_mappings_device` leaves every range's records in one device buffer and `FragmentProfile.add` reduces them
there, pass by pass, so an all-vs-all of any size comes down to 16 bytes per query fragment.

One caveat is part of the semantics.  The records are the mappings computeCGI KEPT: the best of a query fragment per
reference genome, then the best per reference bin.  A fragment that lost its reference bin to a neighbour is absent from that
reference's records, so ``count`` is "references whose hit counts this fragment", not "references where it would map".  The
same (query, fragment, reference) in two records is not detected and counts twice; the mapper never emits that.

There is no CPU path: without a HIP device the calls raise ``RuntimeError``, like every compute entry point.  Not imported by
the package itself (like `clusters`): it needs numpy and torch.
"""
import collections
import ctypes as C
import fractions

import numpy as np
import torch

from ._batch import MAPPING_DTYPE, ROW_DTYPE
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
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
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
        if isinstance(mappings, np.ndarray):
            records = np.ascontiguousarray(mappings, dtype=MAPPING_DTYPE)
            n, ptr, on_device = int(records.shape[0]), records.ctypes.data, 0
        else:
            if mappings.dtype != torch.int32 or mappings.dim() != 2 or mappings.shape[1] != 8 or mappings.device != self.device:
                raise ValueError("device mappings are an int32 [n, 8] tensor on the profile's device")
            records = mappings.contiguous()
            n, ptr, on_device = int(records.shape[0]), records.data_ptr(), 1
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
        mean = self.sum.to(torch.float64) / self.count.clamp(min=1).to(torch.float64) / 2.0 ** 20
        return torch.where(self.count == 0, torch.full_like(mean, float("nan")), mean)

    def summary(self, min_count):
        """Per genome, over its fragments with ``count >= min_count``: ``Summary(fragments, hits, sum)`` -- how many there
        are, the sum of their counts, the sum of their fixed-point sums --, int64 tensors on the profile's device of the
        shape of ``min_count``: int ``[n_queries]`` (`min_count_for`), or ``[c, n_queries]`` for ``c`` thresholds served by one
        walk of the fragments -- the presence curve.  The mean identity of a genome's core is ``sum / hits / 2**20``.  A
        genome without fragments gives zeros.  A negative ``min_count`` raises ``ValueError``."""
        need = np.ascontiguousarray(min_count.cpu().numpy() if hasattr(min_count, "cpu") else min_count)
        if need.dtype.kind not in "iu" or need.ndim not in (1, 2) or need.shape[-1] != self.n_queries or (need.ndim == 2 and need.shape[0] < 1):
            raise ValueError("min_count is int [n_queries], or [c, n_queries] with c >= 1")
        if need.size and (int(need.min()) < 0 or int(need.max()) > np.iinfo(np.int32).max):
            raise ValueError("min_count must not be negative")
        need = need.astype(np.int32)
        n_sets = need.shape[0] if need.ndim == 2 else 1
        out = [torch.zeros(need.shape, dtype=torch.int64, device=self.device) for _ in range(3)]
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            check(lib.fa_profile_summary(C.c_void_p(self.count.data_ptr()), C.c_void_p(self.sum.data_ptr()), self.n_queries,
                                         _ptr(self.fragment_offsets), _ptr(need), n_sets, *[C.c_void_p(x.data_ptr()) for x in out], 1))
        return Summary(*out)

    def core_fraction(self, min_count):
        """The share of every genome's fragments with ``count >= min_count``, float64 of the shape of ``min_count``; NaN for
        a genome without fragments"""
        fragments = self.summary(min_count).fragments
        total = torch.from_numpy(np.diff(self.fragment_offsets)).to(self.device)
        share = fragments.to(torch.float64) / total.clamp(min=1).to(torch.float64)
        return torch.where(total == 0, torch.full_like(share, float("nan")), share)


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
