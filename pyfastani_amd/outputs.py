"""FastANI-style outputs built from the hit table (upstream `outputCGI` / `outputPhylip`,
include/fastani/cgi/compute_core_identity.pxd:39-51 -- not exposed by pyfastani, provided here for all-vs-all runs).

The rows are ``cgi::CGI_Results`` records (``pyfastani_amd._batch.ROW_DTYPE``): query_id, ref_genome_id, count_seq,
total_query_fragments, identity.  The fragment mappings behind them (``pyfastani_amd._batch.MAPPING_DTYPE``, from
`GenomeBatch.query_mappings` / `Mapper.query_draft_mappings`) are what FastANI's ``--visualize`` dumps per fragment.
"""
import numpy as np


def filter_rows(rows, query_lengths, reference_lengths, fragment_length, minimum_fraction=0.2):
    """The reference's hit filter (_fastani.pyx:1121-1132) applied to a whole hit table: keep a row when the mapped
    fragments cover at least ``minimum_fraction`` of the shorter genome (float32 arithmetic, like the reference)."""
    q = np.asarray(query_lengths, dtype=np.float64)[rows["query_id"]]
    r = np.asarray(reference_lengths, dtype=np.float64)[rows["ref_genome_id"]]
    min_len = np.minimum(q, r).astype(np.float32)
    shared = rows["count_seq"].astype(np.float32) * np.float32(fragment_length)
    return rows[shared >= min_len * np.float32(minimum_fraction)]


def identity_matrix(rows, n_queries, n_references, symmetric=False):
    """Dense identity matrix (NaN where there is no hit).  With ``symmetric`` (all-vs-all over one genome set) a cell is
    the mean of the two directions when both exist, as FastANI's matrix output does."""
    m = np.full((n_queries, n_references), np.nan, dtype=np.float64)
    m[rows["query_id"], rows["ref_genome_id"]] = rows["identity"]
    if symmetric:
        if n_queries != n_references:
            raise ValueError("a symmetric matrix needs the same genomes as queries and references")
        both = ~np.isnan(m) & ~np.isnan(m.T)
        either = np.where(np.isnan(m), m.T, m)
        m = np.where(both, (m + m.T) / 2.0, either)
    return m


def write_matrix(path, names, matrix):
    """FastANI's ``--matrix`` layout: the number of genomes, then one line per genome with its name and the identities
    to all earlier genomes (lower triangle), ``NA`` where no hit passed the filters."""
    n = len(names)
    with open(path, "w") as f:
        f.write(f"{n}\n")
        for i in range(n):
            cells = ["NA" if np.isnan(matrix[i, j]) else f"{matrix[i, j]:.6f}" for j in range(i)]
            f.write("\t".join([str(names[i])] + cells) + "\n")


def write_clusters(path, names, labels):
    """The clusters of `pyfastani_amd.clusters.clusters`: one line per genome, in genome order, with its name and the name of
    its label -- the genome of the smallest number in its cluster, which stands for it."""
    labels = labels.cpu().numpy() if hasattr(labels, "cpu") else np.asarray(labels)
    if len(labels) != len(names):
        raise ValueError("one label per name")
    with open(path, "w") as f:
        for name, label in zip(names, labels):
            f.write(f"{name}\t{names[int(label)]}\n")


def write_representatives(path, names, labels, identity):
    """The result of `pyfastani_amd.clusters.representatives`: one line per genome, in genome order, with its name, the name
    of its representative and the symmetric identity of the two (100 for a representative itself).  `write_clusters` takes
    the same labels."""
    labels = labels.cpu().numpy() if hasattr(labels, "cpu") else np.asarray(labels)
    identity = identity.cpu().numpy() if hasattr(identity, "cpu") else np.asarray(identity)
    if len(labels) != len(names) or len(identity) != len(names):
        raise ValueError("one label and one identity per name")
    with open(path, "w") as f:
        for name, label, value in zip(names, labels, identity):
            f.write(f"{name}\t{names[int(label)]}\t{float(value):.6g}\n")


def write_hits(path, query_names, reference_names, rows):
    """FastANI's tabular output: query, reference, ANI, mapped fragments, total query fragments (one line per hit,
    queries in order, hits of a query by decreasing identity)."""
    order = np.lexsort((-rows["identity"], rows["query_id"]))
    with open(path, "w") as f:
        for r in rows[order]:
            f.write(f"{query_names[r['query_id']]}\t{reference_names[r['ref_genome_id']]}\t{r['identity']:.6g}\t"
                    f"{r['count_seq']}\t{r['total_query_fragments']}\n")


def write_best_hits(path, query_names, reference_names, records, offsets):
    """The records of `pyfastani_amd.classify.best_hits` (numpy or tensors) in the layout of `write_hits`, one line per record
    in record order: queries ascending, a query's hits from the best down.  Returns the names of the queries without a
    record -- the unassigned ones."""
    if hasattr(records, "cpu"):
        from .sharding import tensor_to_rows
        records = tensor_to_rows(records)
    offsets = offsets.cpu().numpy() if hasattr(offsets, "cpu") else np.asarray(offsets)
    if len(offsets) != len(query_names) + 1 or int(offsets[-1]) != len(records):
        raise ValueError("one offset per query name and one behind, the last the number of records")
    with open(path, "w") as f:
        for r in records:
            f.write(f"{query_names[r['query_id']]}\t{reference_names[r['ref_genome_id']]}\t{r['identity']:.6g}\t"
                    f"{r['count_seq']}\t{r['total_query_fragments']}\n")
    return [query_names[q] for q in np.nonzero(np.diff(offsets) == 0)[0]]


def write_screen(path, names_a, names_b, records, k):
    """The records of `pyfastani_amd.screen.pairs` (numpy or a tensor) as the columns of ``mash dist`` without its p-value:
    name, name, distance, shared/denom, one line per record in record order.  ``names_b`` is ``names_a`` for the pairs of one
    set."""
    from . import screen
    records = screen.to_records(records)
    with open(path, "w") as f:
        for r, d in zip(records, screen.distance(records, k)):
            f.write(f"{names_a[r['a']]}\t{names_b[r['b']]}\t{d:.6g}\t{r['shared']}/{r['denom']}\n")


def write_containment(path, query_names, reference_names, records, k):
    """The records of `pyfastani_amd.screen.contained` (numpy or a tensor) in the format of `write_screen`: query, reference,
    containment identity, shared/denom, one line per record in record order."""
    from . import screen
    records = screen.to_records(records)
    with open(path, "w") as f:
        for r, i in zip(records, screen.identity(records, k)):
            f.write(f"{query_names[r['a']]}\t{reference_names[r['b']]}\t{i:.6g}\t{r['shared']}/{r['denom']}\n")


def fragment_coordinates(contig_lengths, fragment_length):
    """Where every query fragment lies in its genome: ``(contig, offset)``, two int64 arrays indexed by ``querySeqId``
    (``query_seq_id`` of a mapping).  A contig of length ``n`` holds ``n // fragment_length`` fragments, numbered on from
    the contigs before it (_fastani.pyx:1097,1104); ``contig`` is the index into ``contig_lengths`` as given, short contigs
    included."""
    if fragment_length <= 0:
        raise ValueError("fragment_length must be positive")
    counts = np.asarray(contig_lengths, dtype=np.int64) // int(fragment_length)
    contig = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    first = np.cumsum(counts) - counts                           # querySeqId of every contig's first fragment
    offset = (np.arange(int(counts.sum()), dtype=np.int64) - first[contig]) * int(fragment_length)
    return contig, offset


MAPPING_COLUMNS = ("query", "query_fragment", "query_contig", "query_start", "query_end", "reference", "reference_contig",
                   "reference_start", "identity", "conserved", "sketch_size")


def write_mappings(path, query_names, reference_names, mappings, query_contig_lengths=None, fragment_length=None, append=False):
    """The fragment mappings as a tab-separated table, one line per record in the order given, under a header line naming
    the columns (`MAPPING_COLUMNS`).  ``query_contig_lengths`` (one sequence of contig lengths per query genome, indexed by
    ``query_id``) and ``fragment_length`` place every fragment on its contig; without them the three query coordinate
    columns hold ``NA``.  ``reference_contig`` is the contig's number in the whole reference (``refSeqId``) and
    ``reference_start`` the position on that contig.  This is the project's own layout: upstream's visualisation file is
    written by code outside the reference checkout, and no byte parity with it is claimed.  ``append=True`` adds the lines
    to an existing file and writes no header: the way to write a table range by range (`GenomeBatch.iter_mappings`)."""
    if (query_contig_lengths is None) != (fragment_length is None):
        raise ValueError("query_contig_lengths and fragment_length go together")
    coords = {}
    with open(path, "a" if append else "w") as f:
        if not append:
            f.write("\t".join(MAPPING_COLUMNS) + "\n")
        for r in mappings:
            q, frag = int(r["query_id"]), int(r["query_seq_id"])
            where = ("NA", "NA", "NA")
            if fragment_length is not None:
                if q not in coords:
                    coords[q] = fragment_coordinates(query_contig_lengths[q], fragment_length)
                contig, offset = coords[q]
                where = (int(contig[frag]), int(offset[frag]), int(offset[frag]) + int(fragment_length))
            f.write(f"{query_names[q]}\t{frag}\t{where[0]}\t{where[1]}\t{where[2]}\t{reference_names[r['ref_genome_id']]}\t"
                    f"{r['ref_seq_id']}\t{r['ref_start_pos']}\t{r['identity']:.6g}\t{r['conserved']}\t{r['sketch_size']}\n")
