"""What an all-vs-all is run for, computed where the hit table already is: the symmetric identity of every genome pair and
the groups of genomes above a cut-off (species clusters at 95 %, dereplication at 99 %), by ``fa_table_pairs`` /
``fa_table_clusters`` / ``fa_table_representatives`` / ``fa_table_linkage`` / ``fa_table_dendrogram`` / ``fa_table_medoids`` of the library (include/fastani_hip.h has the semantics; upstream's counterpart is the matrix output,
`outputPhylip`, include/fastani/cgi/compute_core_identity.pxd:39-51 of the reference, and whatever the user clusters it with).

The rows are one genome set mapped against itself: ``query_id`` and ``ref_genome_id`` index the same list of ``n`` genomes,
``n`` being the length of the two length arrays.  ``rows`` is either a ``ROW_DTYPE`` array -- the result is numpy -- or an
``int32 [n_rows, 5]`` torch tensor in HBM (a `ResidentHitTable`'s table, rows left there by
`GenomeBatch.query_rows_device`) -- it is passed by ``data_ptr()`` and the result is a tensor on that device.  There is no
CPU path: without a HIP device the functions raise ``RuntimeError``, like every compute entry point.

Not imported by the package itself (like `outputs`): it needs numpy.
"""
import collections
import ctypes as C

import numpy as np

from ._batch import MERGE_DTYPE, PAIR_DTYPE, ROW_DTYPE
from ._lib import TableParams, check, lib


def _is_tensor(rows):
    return not isinstance(rows, np.ndarray) and hasattr(rows, "data_ptr")


class _Rows:
    """The one reading of a ``rows`` argument: a ``ROW_DTYPE`` array on the host or an int32 ``[n_rows, 5]`` tensor in HBM,
    contiguous and alive for the call, as ``ptr``, ``n_rows`` and ``is_device`` (then ``torch`` and ``device`` are set)."""

    def __init__(self, rows):
        self.torch = self.device = None
        if _is_tensor(rows):
            import torch
            if rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != 5 or not rows.is_cuda:
                raise ValueError("device rows are an int32 [n_rows, 5] tensor in HBM")
            self.torch, self.rows, self.device = torch, rows.contiguous(), rows.device
            self.n_rows, self.ptr = int(rows.shape[0]), self.rows.data_ptr()
            torch.cuda.synchronize(self.device)          # the library runs on a stream of its own: torch's writes are done
        else:
            self.rows = np.ascontiguousarray(rows, dtype=ROW_DTYPE)
            self.n_rows, self.ptr = int(self.rows.shape[0]), self.rows.ctypes.data
        self.is_device = self.torch is not None

    def on_device(self):
        """The calling thread's current device is the one the entry points run on: the tensor's, for the call."""
        import contextlib
        return self.torch.cuda.device(self.device) if self.is_device else contextlib.nullcontext()


class _Table(_Rows):
    """The arguments the entry points share, as ctypes values that stay alive for the call."""

    def __init__(self, rows, query_lengths, reference_lengths, fragment_length, minimum_fraction, min_identity=0.0, reciprocal=False):
        self.qlen = np.ascontiguousarray(query_lengths, dtype=np.uint64)
        self.rlen = np.ascontiguousarray(reference_lengths, dtype=np.uint64)
        if self.qlen.ndim != 1 or self.qlen.shape != self.rlen.shape:
            raise ValueError("query_lengths and reference_lengths are two arrays over the same genomes")
        self.n = int(self.qlen.shape[0])
        self.params = TableParams(float(minimum_fraction), int(fragment_length), float(min_identity), 1 if reciprocal else 0)
        super().__init__(rows)

    def head(self):
        return (C.c_void_p(self.ptr), self.n_rows, 1 if self.is_device else 0, self.n, C.c_void_p(self.qlen.ctypes.data),
                C.c_void_p(self.rlen.ctypes.data), C.byref(self.params))


def pairs(rows, query_lengths, reference_lengths, fragment_length, minimum_fraction=0.2):
    """Every unordered genome pair ``(a, b)``, ``a < b``, with a row that passes the reference's hit filter
    (`outputs.filter_rows`) in at least one direction, sorted by ``(a, b)``: ``PAIR_DTYPE`` records -- an int32
    ``[n_pairs, 6]`` tensor of their words for device rows (`sharding.tensor_to_records` reads it).  ``identity`` is bit for
    bit the cell ``[a, b]`` of ``outputs.identity_matrix(outputs.filter_rows(...), n, n, symmetric=True)``, without the dense
    matrix.  A genome number outside the length arrays, or the same (query, reference) twice, raises ``ValueError``."""
    t = _Table(rows, query_lengths, reference_lengths, fragment_length, minimum_fraction)
    n = C.c_int64(0)
    with t.on_device():
        if t.torch:
            out = t.torch.empty((t.n_rows, 6), dtype=t.torch.int32, device=t.device)       # (a pair has at least one row)
            check(lib.fa_table_pairs(*t.head(), C.c_void_p(out.data_ptr()), t.n_rows, C.byref(n), 1))
            return out[: n.value]
        out = np.empty(t.n_rows, dtype=PAIR_DTYPE)
        check(lib.fa_table_pairs(*t.head(), C.c_void_p(out.ctypes.data), t.n_rows, C.byref(n), 0))
        return out[: n.value].copy()


def clusters(rows, query_lengths, reference_lengths, fragment_length, minimum_fraction=0.2, min_identity=95.0, reciprocal=False,
             stats=None):
    """Single-linkage ANI clusters: the connected components of the pairs whose symmetric identity is at least
    ``min_identity`` (and, with ``reciprocal``, that passed the filter in both directions).  Returns ``labels``, int32
    ``[n]``: the smallest genome number of every genome's cluster; a genome without such a pair labels itself.  ``stats``, a
    dict, receives ``rows`` (surviving the filter), ``pairs``, ``edges``, ``rounds`` (of the component loop) and
    ``n_clusters``."""
    t = _Table(rows, query_lengths, reference_lengths, fragment_length, minimum_fraction, min_identity, reciprocal)
    n_clusters, counters = C.c_int32(0), (C.c_int64 * 4)()
    with t.on_device():
        if t.torch:
            labels = t.torch.empty(t.n, dtype=t.torch.int32, device=t.device)
            check(lib.fa_table_clusters(*t.head(), C.c_void_p(labels.data_ptr()), 1, C.byref(n_clusters), counters))
        else:
            labels = np.empty(t.n, dtype=np.int32)
            check(lib.fa_table_clusters(*t.head(), C.c_void_p(labels.ctypes.data), 0, C.byref(n_clusters), counters))
    if stats is not None:
        stats.update(rows=counters[0], pairs=counters[1], edges=counters[2], rounds=counters[3], n_clusters=n_clusters.value)
    return labels


def average_linkage(rows, query_lengths, reference_lengths, fragment_length, minimum_fraction=0.2, min_identity=95.0, reciprocal=False,
                    missing=0.0, stats=None):
    """Average-linkage (UPGMA) ANI clusters at the cut-off ``min_identity`` (``fa_table_linkage``): the two clusters with the
    largest mean identity over all their genome pairs are merged while that mean is at least ``min_identity``.  A pair
    without a row that passes the filter (with ``reciprocal``: in both directions) counts as ``missing`` -- 0 as in dRep, or
    the floor below which nothing is reported; it must lie below ``min_identity``.  Unlike single linkage the clusters do not
    chain, and unlike `representatives` they do not depend on an order.  Means are compared exactly (fixed point, integers);
    ties go to the pair with the smaller genome numbers.  Returns ``labels``, int32 ``[n]``: the smallest genome number of
    every genome's cluster -- numpy for ``ROW_DTYPE`` rows, a tensor on the rows' device for device rows.  ``stats``, a dict,
    receives ``rows``, ``pairs``, ``present``, ``rounds``, ``merges`` and ``n_clusters``.  Only this partition is returned;
    `dendrogram` returns the tree, to be cut at any higher cut-off.  A negative or NaN ``min_identity`` or ``missing``, or an identity outside [0, 128], raises ``ValueError``; more
    than 2^18 genomes ``NotImplementedError``."""
    t = _Table(rows, query_lengths, reference_lengths, fragment_length, minimum_fraction, min_identity, reciprocal)
    n_clusters, counters = C.c_int32(0), (C.c_int64 * 5)()
    with t.on_device():
        if t.torch:
            labels = t.torch.empty(t.n, dtype=t.torch.int32, device=t.device)
            check(lib.fa_table_linkage(*t.head(), float(missing), C.c_void_p(labels.data_ptr()), 1, C.byref(n_clusters), counters))
        else:
            labels = np.empty(t.n, dtype=np.int32)
            check(lib.fa_table_linkage(*t.head(), float(missing), C.c_void_p(labels.ctypes.data), 0, C.byref(n_clusters), counters))
    if stats is not None:
        stats.update(rows=counters[0], pairs=counters[1], present=counters[2], rounds=counters[3], merges=counters[4],
                     n_clusters=n_clusters.value)
    return labels


def _fixed_cutoff(value):
    """qc as the library forms it from a float32 parameter: rint(value * 2^20), clamped just above the largest weight"""
    return int(min(np.rint(np.float64(np.float32(value)) * 2.0 ** 20), 128.0 * 2.0 ** 20 + 1.0))


class Dendrogram:
    """An average-linkage tree of ``n`` genomes, as `dendrogram` builds it: ``merges``, the merges of the UPGMA walk in the
    order of the walk -- ``MERGE_DTYPE`` records, or an int32 ``[n_merges, 8]`` tensor of their words on the rows' device --,
    ``labels``, the partition at the build cut-off ``min_identity``, and ``missing``.  The tree is known down to
    ``min_identity``: it is a forest with one tree per cluster of ``labels``."""

    def __init__(self, n, merges, labels, min_identity, missing):
        self.n, self.merges, self.labels, self.min_identity, self.missing = n, merges, labels, float(min_identity), float(missing)

    def records(self):
        """``merges`` as ``MERGE_DTYPE`` records on the host"""
        if _is_tensor(self.merges):
            return np.ascontiguousarray(self.merges.detach().cpu().numpy()).reshape(-1).view(MERGE_DTYPE)
        return self.merges

    def identity(self):
        """The mean identity of every merge, float64 ``s / (size_lo * size_hi) / 2**20``: for display -- nothing is decided by
        it, the cuts compare integers."""
        m = self.records()
        return m["s"] / (m["size_lo"].astype(np.float64) * m["size_hi"]) / 2.0 ** 20

    def cut(self, min_identity):
        """The partition at ``min_identity`` (``fa_dendrogram_cut``): labels ``[n]`` for a number, ``[len, n]`` for a
        sequence of them -- what `average_linkage` returns at that cut-off, without another pass over the table.  numpy for
        host merges, a tensor on their device for device merges.  A cut below the build cut-off (compared in fixed point, as
        the library compares) raises ``ValueError``: the tree is not known there."""
        scalar = np.ndim(min_identity) == 0
        cuts = np.ascontiguousarray(np.atleast_1d(np.asarray(min_identity, dtype=np.float32)))
        if cuts.ndim != 1 or len(cuts) < 1:
            raise ValueError("a cut takes one cut-off or a sequence of at least one")
        if np.any(np.isnan(cuts)) or np.any(cuts < 0):
            raise ValueError("min_identity must be a number that is not negative")
        built = _fixed_cutoff(self.min_identity)
        for value in cuts:
            if _fixed_cutoff(value) < built:
                raise ValueError(f"a cut at {float(value)!r} lies below the cut-off the dendrogram was built with, {self.min_identity!r}")
        n_merges = int(self.merges.shape[0])
        head = (n_merges, self.n, C.c_void_p(cuts.ctypes.data), len(cuts))
        if _is_tensor(self.merges) and self.merges.is_cuda:
            import torch
            merges = self.merges.contiguous()
            with torch.cuda.device(merges.device):
                torch.cuda.synchronize(merges.device)          # the library runs on a stream of its own: torch's writes are done
                labels = torch.empty((len(cuts), self.n), dtype=torch.int32, device=merges.device)
                check(lib.fa_dendrogram_cut(C.c_void_p(merges.data_ptr()), head[0], 1, *head[1:], C.c_void_p(labels.data_ptr()), 1, None))
        else:
            merges = np.ascontiguousarray(self.records(), dtype=MERGE_DTYPE)
            labels = np.empty((len(cuts), self.n), dtype=np.int32)
            check(lib.fa_dendrogram_cut(C.c_void_p(merges.ctypes.data), head[0], 0, *head[1:], C.c_void_p(labels.ctypes.data), 0, None))
        return labels[0] if scalar else labels


def dendrogram(rows, query_lengths, reference_lengths, fragment_length, minimum_fraction=0.2, min_identity=95.0, reciprocal=False,
               missing=0.0, stats=None):
    """The average-linkage (UPGMA) tree of the table, built once and cut anywhere (``fa_table_dendrogram``): the arguments, the
    semantics and ``stats`` of `average_linkage`, ``min_identity`` being the BUILD cut-off -- the lowest identity at which
    clusters are still merged, so the lowest at which the tree can be cut (for the whole tree: any value just above
    ``missing``).  Returns a `Dendrogram`; its ``labels`` are those of ``average_linkage`` at ``min_identity``, its ``merges``
    are sorted by decreasing mean identity, exactly and with the tie rule of the walk, so the partition at a higher cut-off is
    a prefix of them: ``cut``.  `outputs.linkage_matrix` and `outputs.write_newick` take the merges."""
    t = _Table(rows, query_lengths, reference_lengths, fragment_length, minimum_fraction, min_identity, reciprocal)
    n_clusters, n_merges, counters = C.c_int32(0), C.c_int64(0), (C.c_int64 * 5)()
    cap = max(t.n - 1, 0)
    with t.on_device():
        if t.torch:
            labels = t.torch.empty(t.n, dtype=t.torch.int32, device=t.device)
            merges = t.torch.empty((cap, 8), dtype=t.torch.int32, device=t.device)
            out = (C.c_void_p(merges.data_ptr()), cap, C.byref(n_merges), C.c_void_p(labels.data_ptr()), 1)
        else:
            labels, merges = np.empty(t.n, dtype=np.int32), np.empty(cap, dtype=MERGE_DTYPE)
            out = (C.c_void_p(merges.ctypes.data), cap, C.byref(n_merges), C.c_void_p(labels.ctypes.data), 0)
        check(lib.fa_table_dendrogram(*t.head(), float(missing), *out, C.byref(n_clusters), counters))
    if stats is not None:
        stats.update(rows=counters[0], pairs=counters[1], present=counters[2], rounds=counters[3], merges=counters[4],
                     n_clusters=n_clusters.value)
    merges = merges[: n_merges.value] if t.torch else merges[: n_merges.value].copy()
    return Dendrogram(t.n, merges, labels, min_identity, missing)


Medoids = collections.namedtuple("Medoids", "labels identity centrality size")


def medoids(rows, query_lengths, reference_lengths, fragment_length, labels, minimum_fraction=0.2, reciprocal=False, missing=0.0,
            bonus=None, stats=None):
    """Centrality and medoids of given clusters (``fa_table_medoids``): ``labels`` is a partition as `clusters`,
    `average_linkage`, `Dendrogram.cut` or `representatives` return it -- int32 ``[n]``, or ``[c, n]`` for ``c`` partitions
    served by one pass over the table; numpy for ``ROW_DTYPE`` rows, a tensor on the rows' device for device rows (mixing the
    two raises ``ValueError``).  A genome's centrality is its mean identity to the other members of its cluster, a pair without
    a row that passes the filter (with ``reciprocal``: in both directions) counting as ``missing``; the medoid of a cluster is
    the member with the largest ``centrality + bonus`` -- ``bonus``, one value per genome in identity points (dRep:
    completeness - 5 x contamination ...), ``None`` for none --, compared exactly in fixed point, ties to the smaller genome
    number.  Returns ``Medoids(labels, identity, centrality, size)``, each of the shape of ``labels``: the medoid of every
    genome's cluster (int32; a medoid labels itself, so `outputs.write_representatives` takes ``labels`` and ``identity``);
    the symmetric identity of the genome and its medoid (float64; 100 for a medoid, NaN where the two have no present pair);
    the centrality (float64, ``sums / (size - 1) / 2**20``, 100 for a cluster of one: for display and for scores the caller
    forms itself -- nothing is decided by it); the size of the cluster (int32).  ``stats``, a dict, receives ``rows``,
    ``pairs``, ``present``, ``inside`` (present pairs inside a cluster, over all partitions) and ``n_clusters`` (a list, one
    per partition).  A label outside ``[0, n)`` or one that is not its own label, a NaN or negative ``missing`` or one above
    128, a NaN ``bonus`` or one beyond 32768 raise ``ValueError``; more than 2^18 genomes ``NotImplementedError``."""
    t = _Table(rows, query_lengths, reference_lengths, fragment_length, minimum_fraction, 0.0, reciprocal)
    if _is_tensor(labels) != t.is_device:
        raise ValueError("labels are numpy for ROW_DTYPE rows and a tensor on the rows' device for device rows")
    if t.is_device:
        if labels.dtype != t.torch.int32 or labels.device != t.device:
            raise ValueError("device labels are an int32 tensor on the rows' device")
        labels = labels.contiguous()
    else:
        labels = np.ascontiguousarray(labels)
        if labels.dtype.kind not in "iu":
            raise ValueError("labels are genome numbers")
        labels = labels.astype(np.int32, copy=False)
    shape = tuple(labels.shape)
    if len(shape) not in (1, 2) or shape[-1] != t.n or (len(shape) == 2 and shape[0] < 1):
        raise ValueError("labels are [n] or [c, n] with c >= 1 over the n genomes of the length arrays")
    n_sets = shape[0] if len(shape) == 2 else 1
    if bonus is not None:
        bonus = np.ascontiguousarray(bonus.cpu().numpy() if hasattr(bonus, "cpu") else bonus, dtype=np.float64)
        if bonus.shape != (t.n,):
            raise ValueError("bonus holds one value per genome")
    bonus_ptr = C.c_void_p(bonus.ctypes.data) if bonus is not None else None
    n_clusters, counters = (C.c_int32 * n_sets)(), (C.c_int64 * 4)()
    with t.on_device():
        if t.torch:
            t.torch.cuda.synchronize(t.device)              # (labels may come from torch's own stream)
            out = [t.torch.empty(shape, dtype=kind, device=t.device) for kind in (t.torch.int32, t.torch.float64, t.torch.int64, t.torch.int32)]
            ptrs = [C.c_void_p(x.data_ptr()) for x in out]
            label_ptr = C.c_void_p(labels.data_ptr())
        else:
            out = [np.empty(shape, dtype=kind) for kind in (np.int32, np.float64, np.int64, np.int32)]
            ptrs = [C.c_void_p(x.ctypes.data) for x in out]
            label_ptr = C.c_void_p(labels.ctypes.data)
        check(lib.fa_table_medoids(*t.head(), float(missing), label_ptr, n_sets, bonus_ptr, *ptrs, 1 if t.is_device else 0, n_clusters,
                                   counters))
    chosen, identity, sums, size = out
    if t.torch:
        centrality = sums.to(t.torch.float64) / (size - 1).clamp(min=1).to(t.torch.float64) / 2.0 ** 20
        centrality = t.torch.where(size == 1, t.torch.full_like(centrality, 100.0), centrality)
    else:
        centrality = np.where(size == 1, 100.0, sums / np.maximum(size - 1, 1).astype(np.float64) / 2.0 ** 20)
    if stats is not None:
        stats.update(rows=counters[0], pairs=counters[1], present=counters[2], inside=counters[3], n_clusters=list(n_clusters))
    return Medoids(chosen, identity, centrality, size)


def _order(order, t):
    """``order`` as a contiguous int32 array over the genomes, or None for genome-number order."""
    if order is None:
        return None
    if isinstance(order, str):
        if order != "length":
            raise ValueError('order is None, "length" or a permutation of the genome numbers')
        return np.lexsort((np.arange(t.n), ~t.qlen)).astype(np.int32)      # longest first (~: descending as unsigned), ties by genome number
    order = np.ascontiguousarray(order.cpu().numpy() if hasattr(order, "cpu") else order)
    if order.shape != (t.n,) or order.dtype.kind not in "iu":
        raise ValueError("order holds one genome number per genome")
    if t.n and (int(order.min()) < 0 or int(order.max()) >= t.n):
        raise ValueError("order is not a permutation of the genome numbers")
    return order.astype(np.int32)


def representatives(rows, query_lengths, reference_lengths, fragment_length, minimum_fraction=0.2, min_identity=95.0,
                    reciprocal=False, order=None, stats=None):
    """Greedy representative clustering (GTDB species clusters, dRep's and galah's dereplicated sets): the genomes are taken in
    ``order`` -- a permutation of the genome numbers, the most preferred first; ``None`` is genome-number order and
    ``"length"`` the longest ``query_lengths`` first, ties by genome number --, a genome becomes a representative unless a pair
    at or above ``min_identity`` (the edges of `clusters`) joins it to an earlier representative, and every other genome joins
    the representative it is closest to (ties to the earlier one).  Unlike single linkage, every genome is within the cut-off
    of the genome that stands for it; which genomes those are depends on ``order``.  Returns ``(labels, identity)``: int32
    ``[n]``, a representative labels itself, and float64 ``[n]``, the symmetric identity to the label (100 for a
    representative) -- numpy for ``ROW_DTYPE`` rows, tensors on the rows' device for device rows.  ``stats``, a dict, receives
    ``rows``, ``pairs``, ``edges``, ``rounds`` (of the selection loop) and ``n_representatives``.  An ``order`` that is no
    permutation, or a negative or NaN ``min_identity``, raises ``ValueError``."""
    t = _Table(rows, query_lengths, reference_lengths, fragment_length, minimum_fraction, min_identity, reciprocal)
    order = _order(order, t)
    order_ptr = C.c_void_p(order.ctypes.data) if order is not None else None
    n_representatives, counters = C.c_int32(0), (C.c_int64 * 4)()
    with t.on_device():
        if t.torch:
            labels = t.torch.empty(t.n, dtype=t.torch.int32, device=t.device)
            identity = t.torch.empty(t.n, dtype=t.torch.float64, device=t.device)
            out = (C.c_void_p(labels.data_ptr()), C.c_void_p(identity.data_ptr()), 1)
        else:
            labels, identity = np.empty(t.n, dtype=np.int32), np.empty(t.n, dtype=np.float64)
            out = (C.c_void_p(labels.ctypes.data), C.c_void_p(identity.ctypes.data), 0)
        check(lib.fa_table_representatives(*t.head(), order_ptr, *out, C.byref(n_representatives), counters))
    if stats is not None:
        stats.update(rows=counters[0], pairs=counters[1], edges=counters[2], rounds=counters[3],
                     n_representatives=n_representatives.value)
    return labels, identity
