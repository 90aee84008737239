"""A screened collection mapped group by group out of ONE resident `Sketch`: the step between `pyfastani_amd.screen`, which
cuts a collection into groups of related genomes, and the reductions of a hit table (`clusters`, `classify`).

    sketch.add_fasta_stream(names, paths)                  # the whole collection, sketched once: 12 bytes per record
    members = screen.partition(screen.groups(screen.pairs(screen.signatures(sketch)), len(names)))
    rows = groups.all_vs_all(sketch, members, paths=paths) # every group indexed, mapped against itself, freed
    labels, identity = clusters.representatives(rows, lengths, lengths, sketch.fragment_length)

A group's index is built from `Sketch.select` (``fa_sketch_select``: the group's records cut out of the collection's on the
device; the collection's sketch is only read), so nothing is sketched twice, and with ``frequency="collection"`` every
group's mapper ignores the hashes the ONE index over the whole collection would ignore (``fa_sketch_frequency``, installed
through ``fa_mapper_set_global_frequency``): candidates, slides and identities only ever look at one reference genome, so
the group's rows are then the rows of the big index for its references -- the argument of the reference-sharded index
(`sharding.build_ref_sharded_mapper`), with groups for shards.  include/fastani_hip.h has the semantics of both entry points.

Everything runs on the device; there is no CPU path.  Not imported by the package itself (like `screen`): it needs numpy
and torch.
"""
import ctypes as C

import numpy as np

from ._batch import ROW_DTYPE
from ._lib import FA_ERR_INVALID, check, lib

INT_MAX = 2**31 - 1


def frequency(sketch, device="cuda"):
    """``(threshold, drop)``: the frequency threshold an index of ``sketch`` would have (``INT_MAX``: nothing is ignored) and
    the distinct hashes with at least that many records -- an int32 tensor of their bit patterns in HBM, ascending as
    unsigned -- without building the index and without touching the sketch.  The pair `sharding.merged_frequency` returns
    and `Mapper._set_global_frequency` takes."""
    import torch
    dev = torch.device(device)
    threshold, n = C.c_int(0), C.c_int64(-1)
    torch.cuda.synchronize(dev)
    with torch.cuda.device(dev):
        cap = 4096                                            # 0.001 % of the distinct hashes at most: one pass is the rule
        drop = torch.empty(cap, dtype=torch.int32, device=dev)
        code = lib.fa_sketch_frequency(C.c_void_p(sketch._h), C.byref(threshold), cap, C.c_void_p(drop.data_ptr()), C.byref(n))
        if code == FA_ERR_INVALID and n.value > cap:          # the buffer was short, and n is what it takes
            cap = n.value
            drop = torch.empty(cap, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            code = lib.fa_sketch_frequency(C.c_void_p(sketch._h), C.byref(threshold), cap, C.c_void_p(drop.data_ptr()), C.byref(n))
        check(code)
    return threshold.value, drop[: n.value]


collection_frequency = frequency       # (all_vs_all has an argument of that name)


def mapper(sketch, members, frequency=None):
    """The `Mapper` over the genomes ``members`` (ascending genome numbers) of ``sketch``, which is left as it is.  With
    ``frequency=(threshold, drop)`` -- what `frequency` returns for the collection -- that filter replaces the group's own
    before the mapper is returned."""
    index = sketch.select(members).index()
    if frequency is not None:
        threshold, drop = frequency
        index._set_global_frequency(threshold, drop)
    return index


def check_partition(partition, n_genomes):
    """The member lists as lists of ints; ``ValueError`` unless they are disjoint, ascending and inside [0, n_genomes)."""
    seen, out = set(), []
    for members in partition:
        members = [int(g) for g in members]
        if any(g < 0 or g >= n_genomes for g in members):
            raise ValueError(f"a group names a genome outside [0, {n_genomes})")
        if any(b <= a for a, b in zip(members, members[1:])):
            raise ValueError("the members of a group must ascend strictly")
        if not seen.isdisjoint(members):
            raise ValueError("the groups of a partition must be disjoint")
        seen.update(members)
        out.append(members)
    return out


def all_vs_all(sketch, partition, genomes=None, paths=None, frequency="collection", min_size=1, chunk=64):
    """Every group of ``partition`` (the member lists of `screen.partition`) mapped against itself: ``ROW_DTYPE`` rows with
    global genome numbers, sorted by ``(query_id, ref_genome_id)`` -- the all-vs-all table of the collection cut to the pairs
    inside a group, as host rows for `clusters.clusters` / `clusters.representatives` / `classify.best_hits`.

    The queries come from ``genomes`` (a list of contig lists indexed by genome number) or from ``paths`` (FASTA files,
    likewise); exactly one is given.  Groups of fewer than ``min_size`` members are skipped.  One group's mapper lives at a
    time.  ``frequency="collection"`` installs the frequency filter of the whole sketch in every group (`frequency`, taken
    once), so that the rows are those of one index over the collection; ``"group"`` leaves every group the threshold of its
    own index.  ``sketch`` is not consumed."""
    if (genomes is None) == (paths is None):
        raise ValueError("exactly one of genomes and paths is given")
    if frequency not in ("collection", "group"):
        raise ValueError('frequency is "collection" or "group"')
    source = genomes if paths is None else paths
    n_genomes = len(source)
    partition = check_partition(partition, n_genomes)
    if n_genomes != len(sketch.names):
        raise ValueError("there is one entry of genomes / paths per genome of the sketch")
    installed = collection_frequency(sketch) if frequency == "collection" else None
    parts = []
    for members in partition:
        if len(members) < max(int(min_size), 1):
            continue
        index = mapper(sketch, members, installed)
        if paths is None:
            batch = index.upload_genomes([genomes[g] for g in members])
        else:
            batch = index.upload_fasta([str(paths[g]) for g in members])
        to_global = np.asarray(members, dtype=np.int32)
        for first in range(0, len(members), chunk):
            rows = batch.query_rows(first, min(chunk, len(members) - first)).copy()
            rows["query_id"] = to_global[rows["query_id"]]
            rows["ref_genome_id"] = to_global[rows["ref_genome_id"]]
            parts.append(rows)
        del batch, index                                       # the group's index leaves HBM before the next is built
    rows = np.concatenate(parts) if parts else np.zeros(0, ROW_DTYPE)
    return rows[np.lexsort((rows["ref_genome_id"], rows["query_id"]))]
