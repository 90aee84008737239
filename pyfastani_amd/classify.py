"""What a batch of queries is mapped against a reference database for, computed where the hit table already is: every
query's ``k`` closest references that pass an identity and an aligned-fraction cut-off, by ``fa_table_best`` of the library
(include/fastani_hip.h has the semantics).  Species assignment is ``min_identity=95, min_aligned_fraction=0.5, k=1``; over
one genome set mapped against itself, ``exclude_self=True`` gives every genome's nearest neighbours.

``query_id`` indexes ``query_lengths`` and ``ref_genome_id`` indexes ``reference_lengths``; the two lists are unrelated and
may differ in length.  ``rows`` is either a ``ROW_DTYPE`` array -- the result is numpy -- or an ``int32 [n_rows, 5]`` torch
tensor in HBM (a `ResidentHitTable`'s table, rows left there by `GenomeBatch.query_rows_device`) -- it is passed by
``data_ptr()`` after a synchronise, the tensor's device is made current for the call, and the result is tensors on that
device.  There is no CPU path: without a HIP device `best_hits` raises ``RuntimeError``, like every compute entry point.

Not imported by the package itself (like `clusters` and `outputs`): it needs numpy.
"""
import ctypes as C

import numpy as np

from ._batch import ROW_DTYPE
from ._lib import BestParams, check, lib
from .clusters import _Rows


def best_hits(rows, query_lengths, reference_lengths, fragment_length, k=1, minimum_fraction=0.2, min_identity=0.0,
              min_aligned_fraction=0.0, exclude_self=False, stats=None):
    """``(records, offsets)``: the ``k`` best surviving rows of every query, and where each query's records lie.

    A row survives the reference's hit filter (`outputs.filter_rows`, ``minimum_fraction``), ``identity >= min_identity``,
    ``count_seq >= total_query_fragments * min_aligned_fraction`` (float32) and, with ``exclude_self``, ``query_id !=
    ref_genome_id``.  A query's survivors are ranked by identity descending, ties by ``ref_genome_id`` ascending -- the order
    of the hits `Mapper.query_draft` returns -- and cut at ``k``.  ``records`` are copies of the input rows, queries
    ascending (``ROW_DTYPE``; an int32 ``[n, 5]`` tensor for device rows); query ``q`` owns ``records[offsets[q]:offsets[q + 1]]``
    (int64 ``[n_queries + 1]``), an empty range when nothing survives.  ``stats``, a dict, receives ``rows`` (surviving),
    ``queries`` (with at least one record) and ``records``.  An id outside the length arrays, or the same (query, reference)
    twice, raises ``ValueError``."""
    qlen = np.ascontiguousarray(query_lengths, dtype=np.uint64)
    rlen = np.ascontiguousarray(reference_lengths, dtype=np.uint64)
    if qlen.ndim != 1 or rlen.ndim != 1:
        raise ValueError("query_lengths and reference_lengths are one-dimensional arrays")
    n_queries, n_references = int(qlen.shape[0]), int(rlen.shape[0])
    params = BestParams(float(minimum_fraction), int(fragment_length), float(min_identity), float(min_aligned_fraction), int(k),
                        1 if exclude_self else 0)
    n, counters = C.c_int64(0), (C.c_int64 * 3)()
    r = _Rows(rows)
    cap = min(r.n_rows, n_queries * max(int(k), 0))
    with r.on_device():
        if r.is_device:
            records = r.torch.empty((cap, 5), dtype=r.torch.int32, device=r.device)
            offsets = r.torch.empty(n_queries + 1, dtype=r.torch.int64, device=r.device)
            out = (C.c_void_p(records.data_ptr()), C.c_void_p(offsets.data_ptr()))
        else:
            records, offsets = np.empty(cap, dtype=ROW_DTYPE), np.empty(n_queries + 1, dtype=np.int64)
            out = (C.c_void_p(records.ctypes.data), C.c_void_p(offsets.ctypes.data))
        check(lib.fa_table_best(C.c_void_p(r.ptr), r.n_rows, 1 if r.is_device else 0, n_queries, n_references, C.c_void_p(qlen.ctypes.data),
                                C.c_void_p(rlen.ctypes.data), C.byref(params), *out, cap, C.byref(n), 1 if r.is_device else 0, counters))
    if stats is not None:
        stats.update(rows=counters[0], queries=counters[1], records=counters[2])
    return (records[: n.value] if r.is_device else records[: n.value].copy()), offsets
