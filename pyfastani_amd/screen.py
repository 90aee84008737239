"""Which genomes of a collection are related at all, found before anything is mapped: every genome reduced to a bottom-``s``
MinHash signature of the minimizer hashes its `Sketch` holds in HBM, signatures compared pair by pair with Mash's merge rule,
the pairs within a Mash distance grouped -- ``fa_screen_signatures`` / ``fa_screen_pairs`` / ``fa_screen_groups`` of the
library (include/fastani_hip.h has the semantics).  A collection too large for one index is cut into its groups this way, and
each group is mapped with what exists: one `Sketch` / `Mapper` / all-vs-all per group.

    sketch.add_fasta_stream(names, paths)
    sigs = screen.signatures(sketch)                       # the sketch stays usable and un-indexed; or sketch.clear(), the
    records = screen.pairs(sigs, max_distance=0.1)         #   next chunk, and Signatures.concat
    members = screen.partition(screen.groups(records, len(sigs)))

The Jaccard estimate of `pairs` collapses when two genomes differ in size (a contig, a plasmid, an incomplete genome against
its complete relative).  The containment road is for those: ``fa_screen_contents`` / ``fa_screen_contained``, what ``mash
screen`` computes.

    contents = screen.contents(sketch)                     # every genome's FULL distinct hash set, one sorted directory in HBM
    found = screen.contained(query_sigs, contents, min_identity=0.9)       # a: query, b: genome; `identity` of each record
    records = screen.fold(screen.contained(sigs, contents))                # a collection in itself, as triangular records
    one = screen.contained(query_sigs, contents, winner_take_all=True, weights="length")     # every hash credited to ONE genome

A query of a well-sampled species is contained in every one of its strains.  With ``winner_take_all`` every hash of the query
is credited to one genome only -- of those that hold it the one holding the most of the query's hashes (``first``, the plain
``shared``); ties go to the larger weight, then to the smaller genome number -- and a record carries what its genome *won*:
redundant relatives fall to what they alone explain and drop below the cut-off.  The rule is this library's integer
restatement of ``mash screen -w`` (``fa_screen_contained_winner``); it has not been checked against the Mash program.

Queries need no `Sketch` of their own: a `GenomeBatch` is reduced to signatures from the fragments it already holds in HBM
(``fa_genomes_signatures``), pass by pass in bounded memory, and is then mapped as it is.

    batch = mapper.upload_genomes(queries)                 # once
    query_sigs = screen.signatures(batch, size=1000)       # names: the genome numbers, or names=; first= / count= take a range
    found = screen.contained(query_sigs, contents)         # ... and batch.query() maps the same upload

The signature is that of the genome's *winnowed minimizers*, not of all its k-mers, and so is every statistic here, the
winner-take-all one included: the distances are Mash-like at the sketch's ``k``, not those of the Mash program.  A batch's
signature is one step further away: a batch keeps only the whole fragments of each contig and its windows do not cross fragment
seams, so a genome's hash set is a *subset* of what a `Sketch` holds for the same contigs (and equals that of a `Sketch` to
which every fragment was added as a contig of its own): the two signatures are close, not identical.  Everything but `fold` runs on the device; there is no CPU path, and without a HIP device
the functions raise ``RuntimeError`` like every compute entry point.

Not imported by the package itself (like `clusters` and `classify`): it needs numpy.
"""
import ctypes as C
import math

import numpy as np

from ._lib import FA_ERR_INVALID, check, lib

# fa_screen_pair: ``shared`` of the first ``denom`` elements of the two signatures' union occur in both
SCREEN_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("shared", "<i4"), ("denom", "<i4")])
assert SCREEN_DTYPE.itemsize == 16

JACCARD_DENOMINATOR = 1 << 20
MAX_SIZE = 4096


class Signatures:
    """The signatures of ``len(names)`` genomes: ``sig`` int32 ``[n, size]`` (the bits of unsigned 32-bit hashes, ascending
    as unsigned, zero from the count on) and ``count`` int32 ``[n]``, both in HBM, with the genomes' ``names`` and the
    k-mer size ``k`` of the sketch they came from."""

    def __init__(self, sig, count, names, k):
        if sig.dim() != 2 or count.dim() != 1 or sig.shape[0] != count.shape[0] or len(names) != sig.shape[0]:
            raise ValueError("sig is [n, size], count [n], and there is one name per genome")
        self.sig, self.count, self.names, self.k = sig, count, list(names), int(k)

    def __len__(self):
        return len(self.names)

    @property
    def size(self):
        return int(self.sig.shape[1])

    @property
    def device(self):
        return self.sig.device

    @staticmethod
    def concat(parts):
        """One set out of several of the same size, ``k`` and device, genomes in the order given: the way to screen a
        collection that is sketched chunk by chunk (``add_fasta_stream`` + `signatures` + ``clear``)."""
        import torch
        parts = list(parts)
        if not parts:
            raise ValueError("nothing to join")
        if len({(p.size, p.k, p.device) for p in parts}) != 1:
            raise ValueError("signature sets of different size, k or device do not compare")
        return Signatures(torch.cat([p.sig for p in parts]), torch.cat([p.count for p in parts]), sum((p.names for p in parts), []),
                          parts[0].k)


def signatures(source, size=1000, device="cuda", names=None, first=0, count=None, pass_fragments=0, stats=None):
    """The bottom-``size`` signatures (1 <= size <= 4096) of every genome of ``source``.

    A `Sketch`: from the records `Sketch._export_records` copies HBM to HBM; the sketch is left as it is, un-indexed.
    ``names``, ``first`` and ``count`` belong to the other source and raise ``ValueError`` here.

    A `GenomeBatch`: of its genomes ``[first, first + count)``, from the fragments the batch holds already, pass by pass in
    bounded memory on the device of the batch's mapper (``fa_genomes_signatures``; ``device`` plays no part) -- queries are
    uploaded once, screened and mapped.  ``names`` default to the genome numbers as strings, ``k`` is the mapper's.
    ``pass_fragments`` sets the fragments per pass of this call (0: the library's, ``FA_PASS_FRAGMENTS``); the result does not
    depend on it.  ``stats``, a dict, receives ``fragments`` and ``passes``, and ``k1_us`` / ``device_us`` (the device time of
    the sketch kernel and of all passes; 0 unless the mapper's stage events are on).  The call is not a query: the mapper's
    timings and stage getters go on speaking of its last query."""
    if not 1 <= int(size) <= MAX_SIZE:
        raise ValueError(f"the signature size must be in [1, {MAX_SIZE}]")
    if hasattr(source, "_export_records"):
        if names is not None or first != 0 or count is not None:
            raise ValueError("names, first and count select genomes of a GenomeBatch: a Sketch is taken whole, under its own names")
        return _sketch_signatures(source, size, device)
    return _batch_signatures(source, int(size), names, int(first), count, int(pass_fragments), stats)


def _sketch_signatures(sketch, size, device):
    import torch
    rec, (lengths, sbf, counter) = sketch._export_records(device)
    rec = rec.contiguous()
    n, n_records = len(sbf), int(rec.shape[1])
    sbf = np.ascontiguousarray(sbf, dtype=np.int32)
    sig = torch.empty((n, int(size)), dtype=torch.int32, device=rec.device)
    count = torch.empty(n, dtype=torch.int32, device=rec.device)
    torch.cuda.synchronize(rec.device)                   # the library runs on a stream of its own: torch's writes are done
    with torch.cuda.device(rec.device):
        check(lib.fa_screen_signatures(C.c_void_p(rec[0].data_ptr()), C.c_void_p(rec[1].data_ptr()), n_records,
                                       C.c_void_p(sbf.ctypes.data), n, int(size), C.c_void_p(sig.data_ptr()), C.c_void_p(count.data_ptr())))
    return Signatures(sig, count, sketch.names, sketch.k)


def _batch_signatures(batch, size, names, first, count, pass_fragments, stats):
    n = len(batch)
    count = n - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > n:
        raise ValueError("genome range out of bounds")
    names = [str(g) for g in range(first, first + count)] if names is None else list(names)
    if len(names) != count:
        raise ValueError("there is one name per genome of the range")
    if pass_fragments < 0:
        raise ValueError("pass_fragments must not be negative")
    import torch
    mapper = batch._mapper
    where = mapper._torch_device()
    sig = torch.empty((count, size), dtype=torch.int32, device=where)
    tally = torch.empty(count, dtype=torch.int32, device=where)
    counters = (C.c_int64 * 4)()
    torch.cuda.synchronize(where)                        # the library runs on a stream of the mapper's: torch's writes are done
    with torch.cuda.device(where):
        check(lib.fa_genomes_signatures(C.c_void_p(mapper._h), C.c_void_p(batch._h), first, count, size, pass_fragments,
                                        C.c_void_p(sig.data_ptr()) if count else None, C.c_void_p(tally.data_ptr()) if count else None, counters))
    if stats is not None:
        stats.update(fragments=counters[0], passes=counters[1], k1_us=counters[2], device_us=counters[3])
    return Signatures(sig, tally, names, mapper.k)


def jaccard_cutoff(max_distance, k):
    """``(jn, jd)``: the Jaccard index of Mash distance ``max_distance`` at k-mer size ``k``, ``1 / (2 exp(k d) - 1)``, as a
    fraction over 2**20 rounded DOWN (and one step further, for the rounding of the float64 arithmetic itself), so that the
    integer filter of the device keeps every pair the exact float64 cut by `distance` keeps."""
    if not max_distance >= 0.0:
        raise ValueError("max_distance must be a number that is not negative")
    if max_distance >= 1.0:                              # (a pair that shares nothing has distance 1.0)
        return 0, JACCARD_DENOMINATOR
    j_min = 1.0 / (2.0 * math.exp(int(k) * float(max_distance)) - 1.0)
    return max(0, min(JACCARD_DENOMINATOR, int(math.floor(j_min * JACCARD_DENOMINATOR)) - 1)), JACCARD_DENOMINATOR


def distance(records, k):
    """Mash's distance ``-ln(2 j / (1 + j)) / k`` of every record, ``j = shared / denom``, in float64: 1.0 for
    ``shared == 0`` and 0.0 for ``j == 1``.  ``records`` are ``SCREEN_DTYPE`` or an int32 ``[n, 4]`` tensor."""
    records = to_records(records)
    shared, denom = records["shared"].astype(np.float64), records["denom"].astype(np.float64)
    out = np.ones(len(records), dtype=np.float64)
    some = shared > 0
    j = shared[some] / denom[some]
    out[some] = np.where(j >= 1.0, 0.0, -np.log(2.0 * j / (1.0 + j)) / float(k))
    return out


def to_records(records):
    """``SCREEN_DTYPE`` records of an int32 ``[n, 4]`` tensor (or of records, unchanged)"""
    if hasattr(records, "cpu"):
        return np.ascontiguousarray(records.cpu().numpy()).view(SCREEN_DTYPE).reshape(-1)
    return np.ascontiguousarray(records, dtype=SCREEN_DTYPE)


def pairs(a, b=None, max_distance=0.1, device=False, stats=None):
    """The genome pairs within Mash distance ``max_distance``, sorted by ``(a, b)``: ``SCREEN_DTYPE`` records, or with
    ``device=True`` the int32 ``[n, 4]`` tensor of their words in HBM.  With one set (``b is None``) the pairs ``a < b`` of
    the set; with two, every (genome of ``a``, genome of ``b``).  The device filters by the integer Jaccard cut-off of
    `jaccard_cutoff`, which loses nothing; the survivors are then cut exactly by `distance` in float64.  ``stats``, a dict,
    receives ``evaluated`` and ``kept`` (by the device filter)."""
    import torch
    other = a if b is None else b
    if (other.size, other.k, other.device) != (a.size, a.k, a.device):
        raise ValueError("signature sets of different size, k or device do not compare")
    jn, jd = jaccard_cutoff(max_distance, a.k)
    sig_a, count_a, sig_b, count_b = a.sig.contiguous(), a.count.contiguous(), other.sig.contiguous(), other.count.contiguous()
    if b is None:
        sig_b, count_b = sig_a, count_a
    head = (C.c_void_p(sig_a.data_ptr()), C.c_void_p(count_a.data_ptr()), len(a), C.c_void_p(sig_b.data_ptr()),
            C.c_void_p(count_b.data_ptr()), len(other), a.size, 1 if b is None else 0, jn, jd)
    n, counters = C.c_int64(-1), (C.c_int64 * 2)()
    total = len(a) * (len(a) - 1) // 2 if b is None else len(a) * len(other)
    cap = min(total, max(4096, 16 * (len(a) + len(other))))           # a screen keeps few pairs: one pass is the rule
    torch.cuda.synchronize(a.device)
    with torch.cuda.device(a.device):
        out = torch.empty((cap, 4), dtype=torch.int32, device=a.device)
        code = lib.fa_screen_pairs(*head, C.c_void_p(out.data_ptr()), cap, C.byref(n), 1, counters)
        if code == FA_ERR_INVALID and n.value > cap:                  # the buffer was short, and n is what it takes
            out = torch.empty((n.value, 4), dtype=torch.int32, device=a.device)
            torch.cuda.synchronize(a.device)
            code = lib.fa_screen_pairs(*head, C.c_void_p(out.data_ptr()), n.value, C.byref(n), 1, counters)
        check(code)
        out = out[: n.value]
    if stats is not None:
        stats.update(evaluated=counters[0], kept=counters[1])
    records = to_records(out)
    keep = distance(records, a.k) <= float(max_distance)
    if device:
        return out if keep.all() else out[torch.from_numpy(keep).to(out.device)]
    return records[keep]


# ---- the containment road ----------------------------------------------------------------------------------------------
class Contents:
    """The contents of a collection of ``len(names)`` genomes: its distinct (hash, genome) pairs as ``hash`` and ``genome``,
    int32 ``[m]`` each (``hash`` holds the bits of unsigned 32-bit values), in HBM and sorted by hash as unsigned, then by
    genome -- the directory `contained` looks signatures up in -- with the genomes' ``names`` and the k-mer size ``k``.
    ``lengths``, when known, is every genome's total length as numpy int64 -- as the sketch counts it, every contig in whole
    fragments -- the weights ``"length"`` of `contained`."""

    def __init__(self, hash, genome, names, k, lengths=None):
        if hash.dim() != 1 or genome.dim() != 1 or hash.shape[0] != genome.shape[0]:
            raise ValueError("hash and genome are [m], one of each per entry")
        self.hash, self.genome, self.names, self.k = hash, genome, list(names), int(k)
        self.lengths = None if lengths is None else np.ascontiguousarray(lengths).astype(np.int64)
        if self.lengths is not None and self.lengths.shape != (len(self.names),):
            raise ValueError("there is one length per genome")

    def __len__(self):
        return len(self.names)

    @property
    def entries(self):
        return int(self.hash.shape[0])

    @property
    def device(self):
        return self.hash.device


def contents(sketch, device="cuda"):
    """The `Contents` of every genome of ``sketch``, from the records `Sketch._export_records` copies HBM to HBM: the sketch
    is left as it is, un-indexed.  Where a `Signatures` keeps the bottom ``size`` of a genome's hashes, this keeps them all."""
    import torch
    rec, (lengths, sbf, counter) = sketch._export_records(device)
    rec = rec.contiguous()
    n, n_records = len(sbf), int(rec.shape[1])
    sbf = np.ascontiguousarray(sbf, dtype=np.int32)
    ent_hash = torch.empty(n_records, dtype=torch.int32, device=rec.device)          # n_records entries always suffice
    ent_genome = torch.empty(n_records, dtype=torch.int32, device=rec.device)
    m = C.c_int64(0)
    torch.cuda.synchronize(rec.device)                   # the library runs on a stream of its own: torch's writes are done
    with torch.cuda.device(rec.device):
        check(lib.fa_screen_contents(C.c_void_p(rec[0].data_ptr()), C.c_void_p(rec[1].data_ptr()), n_records, C.c_void_p(sbf.ctypes.data), n,
                                     C.c_void_p(ent_hash.data_ptr()), C.c_void_p(ent_genome.data_ptr()), n_records, C.byref(m)))
    return Contents(ent_hash[: m.value].clone(), ent_genome[: m.value].clone(), sketch.names, sketch.k, lengths)


def containment_cutoff(min_identity, k):
    """``(cn, cd)``: the containment of identity ``min_identity`` at k-mer size ``k``, ``min_identity ** k``, as a fraction
    over 2**20 rounded DOWN (and one step further, for the rounding of the float64 arithmetic itself), so that the integer
    filter of the device keeps every pair the exact float64 cut by `identity` keeps: a pair below ``cn / cd`` has a
    containment at least 2**-20 below ``min_identity ** k``, hence (the k-th root has slope >= 1 / k on [0, 1]) an identity
    at least 2**-20 / k below ``min_identity``, far beyond what float64 rounds."""
    if not 0.0 <= min_identity <= 1.0:
        raise ValueError("min_identity must be a number in [0, 1]")
    c_min = float(min_identity) ** int(k)
    return max(0, min(JACCARD_DENOMINATOR, int(math.floor(c_min * JACCARD_DENOMINATOR)) - 1)), JACCARD_DENOMINATOR


def identity(records, k):
    """``(shared / denom) ** (1 / k)`` of every record in float64 -- the identity at which a k-mer of the query survives in
    the reference with probability ``shared / denom`` (Mash's containment index) -- and 0.0 for ``shared == 0``."""
    records = to_records(records)
    shared, denom = records["shared"].astype(np.float64), records["denom"].astype(np.float64)
    out = np.zeros(len(records), dtype=np.float64)
    some = shared > 0
    out[some] = (shared[some] / denom[some]) ** (1.0 / float(k))
    return out


def _winner_weights(weights, contents):
    """``weights`` of `contained` as contiguous int32 numpy, one per genome of ``contents``"""
    if isinstance(weights, str):
        if weights != "length":
            raise ValueError('weights are a sequence of integers, or "length"')
        if contents.lengths is None:
            raise ValueError("these contents do not know their genomes' lengths")
        return np.minimum(contents.lengths, np.iinfo(np.int32).max).astype(np.int32)
    values = np.asarray(weights.cpu() if hasattr(weights, "cpu") else weights)
    if values.shape != (len(contents),) or not (np.issubdtype(values.dtype, np.integer) or values.size == 0):
        raise ValueError("weights are one integer per genome of the contents")
    if values.size and (int(values.min()) < 0 or int(values.max()) > np.iinfo(np.int32).max):
        raise ValueError("a weight is an integer in [0, 2**31 - 1]")
    return np.ascontiguousarray(values, dtype=np.int32)


def contained(sigs, contents, min_identity=0.9, device=False, stats=None, winner_take_all=False, weights=None):
    """The (signature of ``sigs``, genome of ``contents``) pairs of containment identity at least ``min_identity``, sorted by
    ``(a, b)``: ``SCREEN_DTYPE`` records with ``shared`` of the signature's ``denom`` elements found in the genome, or with
    ``device=True`` the int32 ``[n, 4]`` tensor of their words in HBM.  The device filters by the integer cut-off of
    `containment_cutoff`, which loses nothing; the survivors are then cut exactly by `identity` in float64.  ``stats``, a
    dict, receives ``evaluated``, ``kept`` (by the device filter) and ``visited`` (directory entries).

    With ``winner_take_all`` every element of a signature is credited to one genome only (the module docstring has the rule)
    and ``shared`` is what the genome won; ``stats`` also receives ``assigned``, the elements that found a genome.
    ``weights`` break the ties of that rule: ``None`` (none), one non-negative integer per genome (a sequence, numpy or a
    tensor), or ``"length"`` for ``contents.lengths`` clipped to int32 -- Mash's own tie rule, the longer reference."""
    import torch
    if (sigs.k, sigs.device) != (contents.k, contents.device):
        raise ValueError("signatures and contents of different k or device do not compare")
    if weights is not None and not winner_take_all:
        raise ValueError("weights break the ties of winner_take_all and mean nothing without it")
    if weights is not None:
        weights = _winner_weights(weights, contents)
    cn, cd = containment_cutoff(min_identity, sigs.k)
    sig, count = sigs.sig.contiguous(), sigs.count.contiguous()
    ent_hash, ent_genome = contents.hash.contiguous(), contents.genome.contiguous()
    head = (C.c_void_p(sig.data_ptr()), C.c_void_p(count.data_ptr()), len(sigs), sigs.size, C.c_void_p(ent_hash.data_ptr()),
            C.c_void_p(ent_genome.data_ptr()), contents.entries, len(contents), cn, cd)
    call = lib.fa_screen_contained
    if winner_take_all:
        call = lib.fa_screen_contained_winner
        d_weights = None if weights is None else torch.from_numpy(weights).to(sigs.device)
        head = head[:8] + (None if d_weights is None or not len(contents) else C.c_void_p(d_weights.data_ptr()),) + head[8:]
    n, counters = C.c_int64(-1), (C.c_int64 * 4)()
    cap = min(len(sigs) * len(contents), max(4096, 16 * (len(sigs) + len(contents))))      # a screen keeps few pairs: one pass is the rule
    torch.cuda.synchronize(sigs.device)
    with torch.cuda.device(sigs.device):
        out = torch.empty((cap, 4), dtype=torch.int32, device=sigs.device)
        code = call(*head, C.c_void_p(out.data_ptr()), cap, C.byref(n), 1, counters)
        if code == FA_ERR_INVALID and n.value > cap:                  # the buffer was short, and n is what it takes
            out = torch.empty((n.value, 4), dtype=torch.int32, device=sigs.device)
            torch.cuda.synchronize(sigs.device)
            code = call(*head, C.c_void_p(out.data_ptr()), n.value, C.byref(n), 1, counters)
        check(code)
        out = out[: n.value]
    if stats is not None:
        stats.update(evaluated=counters[0], kept=counters[1], visited=counters[2])
        if winner_take_all:
            stats.update(assigned=counters[3])
    records = to_records(out)
    keep = identity(records, sigs.k) >= float(min_identity)
    if device:
        return out if keep.all() else out[torch.from_numpy(keep).to(out.device)]
    return records[keep]


def fold(records):
    """The records of a collection contained in itself (`contained` of its own signatures) as triangular records `groups`
    takes: ``a == b`` is dropped, and of the two directions of an unordered pair the one with the larger ``shared / denom``
    is kept (compared by integer cross-multiplication; on a tie the record whose own ``a < b``), written as
    ``(min, max, shared, denom)`` and sorted by ``(a, b)``.  On the host, with numpy."""
    records = to_records(records)
    records = records[records["a"] != records["b"]]
    lo, hi = np.minimum(records["a"], records["b"]), np.maximum(records["a"], records["b"])
    forward = records["a"] < records["b"]
    order = np.lexsort((~forward, hi, lo))                            # by (lo, hi), the record whose own a < b first
    records, lo, hi = records[order], lo[order], hi[order]
    first = np.ones(len(records), dtype=bool)
    first[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    take = np.nonzero(first)[0]
    other = np.minimum(take + 1, len(records) - 1)
    paired = (other != take) & ~first[other]                          # the pair has a second record, right behind the first
    s0, d0 = records["shared"][take].astype(np.int64), records["denom"][take].astype(np.int64)
    s1, d1 = records["shared"][other].astype(np.int64), records["denom"][other].astype(np.int64)
    take = np.where(paired & (s1 * d0 > s0 * d1), other, take)        # the second only when strictly larger
    out = np.zeros(len(take), dtype=SCREEN_DTYPE)
    out["a"], out["b"], out["shared"], out["denom"] = lo[take], hi[take], records["shared"][take], records["denom"][take]
    return out


def groups(records, n, max_distance=None, k=None):
    """``labels``, int32 ``[n]``: the smallest genome number of every genome's group, the groups being the connected
    components of the triangular ``records`` -- of those within ``max_distance`` when one is given (``k``, the k-mer size,
    is then needed for `distance`).  A tensor for records in HBM, numpy otherwise."""
    if max_distance is not None:
        if k is None:
            raise ValueError("a cut by max_distance needs the k-mer size k")
        keep = distance(records, k) <= float(max_distance)
        if hasattr(records, "cpu"):
            import torch
            records = records[torch.from_numpy(keep).to(records.device)]
        else:
            records = np.ascontiguousarray(records, dtype=SCREEN_DTYPE)[keep]
    n_groups = C.c_int32(0)
    if hasattr(records, "cpu"):
        import torch
        if records.dtype != torch.int32 or records.dim() != 2 or records.shape[1] != 4 or not records.is_cuda:
            raise ValueError("device records are an int32 [n, 4] tensor in HBM")
        records = records.contiguous()
        labels = torch.empty(int(n), dtype=torch.int32, device=records.device)
        torch.cuda.synchronize(records.device)
        with torch.cuda.device(records.device):
            check(lib.fa_screen_groups(C.c_void_p(records.data_ptr()), int(records.shape[0]), 1, int(n), C.c_void_p(labels.data_ptr()), 1,
                                       C.byref(n_groups)))
        return labels
    records = np.ascontiguousarray(records, dtype=SCREEN_DTYPE)
    labels = np.empty(int(n), dtype=np.int32)
    check(lib.fa_screen_groups(C.c_void_p(records.ctypes.data), len(records), 0, int(n), C.c_void_p(labels.ctypes.data), 0, C.byref(n_groups)))
    return labels


def partition(labels):
    """The member lists of the groups, the largest group first (ties: the smaller label first), members ascending."""
    labels = labels.cpu().numpy() if hasattr(labels, "cpu") else np.asarray(labels)
    members = {}
    for g, label in enumerate(labels.tolist()):
        members.setdefault(label, []).append(g)
    return [members[label] for label in sorted(members, key=lambda label: (-len(members[label]), label))]
