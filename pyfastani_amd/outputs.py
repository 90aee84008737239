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
    the same labels.  The ``labels`` and ``identity`` of one partition of `pyfastani_amd.clusters.medoids` are written the same
    way; a member without a row with its medoid has a NaN identity, printed as ``nan``."""
    labels = labels.cpu().numpy() if hasattr(labels, "cpu") else np.asarray(labels)
    identity = identity.cpu().numpy() if hasattr(identity, "cpu") else np.asarray(identity)
    if len(labels) != len(names) or len(identity) != len(names):
        raise ValueError("one label and one identity per name")
    with open(path, "w") as f:
        for name, label, value in zip(names, labels, identity):
            f.write(f"{name}\t{names[int(label)]}\t{float(value):.6g}\n")


def _merge_records(merges):
    """the merges of a `pyfastani_amd.clusters.Dendrogram` -- ``MERGE_DTYPE`` records, or the int32 ``[n_merges, 8]`` tensor of
    their words -- as records on the host, with every merge's mean identity in float64"""
    if hasattr(merges, "cpu"):
        from ._batch import MERGE_DTYPE
        merges = np.ascontiguousarray(merges.detach().cpu().numpy()).reshape(-1).view(MERGE_DTYPE)
    merges = np.asarray(merges)
    identity = merges["s"] / (merges["size_lo"].astype(np.float64) * merges["size_hi"]) / 2.0 ** 20
    return merges, identity


def linkage_matrix(merges, n):
    """scipy's linkage matrix ``Z``, float64 ``[n - 1, 4]``, of the merges of a dendrogram over ``n`` genomes
    (`pyfastani_amd.clusters.dendrogram`): row ``i`` holds the ids of the two clusters merge ``i`` joins -- a genome number,
    or ``n + j`` for the result of merge ``j``; the smaller id first --, their distance ``100 - identity`` and the number of
    genomes of the result.  `scipy.cluster.hierarchy.fcluster` and `dendrogram` take it.  A list that is not exactly
    ``n - 1`` merges long is a forest (the tree was built with a cut-off above its root) and raises ``ValueError``."""
    merges, identity = _merge_records(merges)
    if n < 1 or len(merges) != n - 1:
        raise ValueError(f"a linkage matrix of {n} genomes has {n - 1} merges, not {len(merges)}: build the dendrogram with a lower cut-off")
    z = np.zeros((len(merges), 4), dtype=np.float64)
    node = np.arange(n)                                             # the id of the cluster a label stands for now
    for i, m in enumerate(merges):
        a, b = int(node[m["lo"]]), int(node[m["hi"]])
        z[i] = (min(a, b), max(a, b), 100.0 - identity[i], int(m["size_lo"]) + int(m["size_hi"]))
        node[m["lo"]] = n + i
    return z


def _newick_name(name):
    name = str(name)
    if any(c.isspace() or c in "()[]':;," for c in name):
        return "'" + name.replace("'", "''") + "'"
    return name


def write_newick(path, names, merges, n):
    """The merges of a dendrogram over ``n`` genomes (`pyfastani_amd.clusters.dendrogram`) as Newick: one tree per cluster of
    the list -- a list built with a cut-off above its root is a forest --, one per line, in the order of the clusters' labels;
    a genome no merge touches is written ``name;``.  The subtree of the smaller label comes first.  A node's height is
    ``(100 - identity) / 2``, so two leaves are ``100 - identity`` of the merge that joined them apart; leaves are at 0.
    Heights are rounded to six decimals and a branch length is the difference of two of them, written with six decimals: the
    lengths from a node down to every leaf below it add up to the same number.  They are never negative, because the list is
    sorted.  A name with whitespace or one of ``()[]':;,`` is single-quoted, with ``'`` doubled."""
    merges, identity = _merge_records(merges)
    if len(names) != n:
        raise ValueError("one name per genome")
    height = [0] * n + [int(round((100.0 - float(v)) / 2.0 * 1e6)) for v in identity]      # in units of 1e-6; leaves, then merges
    children = {}
    node = list(range(n))
    absorbed = [False] * n
    for i, m in enumerate(merges):
        lo, hi = int(m["lo"]), int(m["hi"])
        children[n + i] = (node[lo], node[hi])
        node[lo] = n + i
        absorbed[hi] = True
    with open(path, "w") as f:
        for label in range(n):
            if absorbed[label]:
                continue
            # depth first without recursion (a tree can be n - 1 deep): a node, or a piece of text to write on the way back
            text, stack = [], [node[label]]
            while stack:
                item = stack.pop()
                if isinstance(item, str):
                    text.append(item)
                elif item < n:
                    text.append(_newick_name(names[item]))
                else:
                    first, second = children[item]
                    lengths = [height[item] - height[child] for child in (first, second)]
                    pieces = [f":{d // 1000000}.{d % 1000000:06d}" if d >= 0 else f":-{-d // 1000000}.{-d % 1000000:06d}" for d in lengths]
                    text.append("(")
                    stack += [pieces[1] + ")", second, pieces[0] + ",", first]
            f.write("".join(text) + ";\n")


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


PROFILE_COLUMNS = ("genome", "contig", "start", "end", "count", "mean_identity", "lowest_identity")


def write_fragment_profile(path, names, count, sum, lowest, contig_lengths, fragment_length):
    """A `pyfastani_amd.conservation.FragmentProfile` as a tab-separated table, one line per query fragment in profile order
    under a header line naming the columns (`PROFILE_COLUMNS`): the genome, the fragment's contig (its index into the
    genome's ``contig_lengths`` as given, short contigs included), start and end on it (`fragment_coordinates`), the number of
    counted records, and their mean (``sum / count / 2**20``) and lowest identity -- ``NA`` for both where the count is 0.
    ``count``, ``sum`` and ``lowest`` are the profile's three arrays (numpy or tensors); ``contig_lengths`` holds one sequence
    of contig lengths per genome, in the order of ``names``."""
    count, sum, lowest = (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in (count, sum, lowest))
    if len(names) != len(contig_lengths):
        raise ValueError("one sequence of contig lengths per genome name")
    coords = [fragment_coordinates(lengths, fragment_length) for lengths in contig_lengths]
    if not (len(count) == len(sum) == len(lowest) == int(np.sum([len(c) for c, _ in coords], dtype=np.int64))):
        raise ValueError("the profile holds one entry per fragment of the genomes")
    at = 0
    with open(path, "w") as f:
        f.write("\t".join(PROFILE_COLUMNS) + "\n")
        for name, (contig, offset) in zip(names, coords):
            for k in range(len(contig)):
                c = int(count[at])
                values = (f"{int(sum[at]) / c / 2.0 ** 20:.6g}", f"{float(lowest[at]):.6g}") if c else ("NA", "NA")
                f.write(f"{name}\t{int(contig[k])}\t{int(offset[k])}\t{int(offset[k]) + int(fragment_length)}\t{c}\t{values[0]}\t{values[1]}\n")
                at += 1


def write_reference_profile(path, names, profile):
    """A `pyfastani_amd.conservation.ReferenceProfile` as a tab-separated table, one line per reference bin in profile order
    under a header line naming the columns (`PROFILE_COLUMNS`): the reference genome, the bin's contig numbered inside its
    genome, start (``bin * bin_length``) and end (start + ``bin_length``) on it, the number of counted records, and their mean
    (``sum / count / 2**20``) and lowest identity -- ``NA`` for both where the count is 0.  ``profile`` is anything with
    ``bin_length``, ``contig_bin``, ``contig_genome``, ``count``, ``sum`` and ``lowest`` (numpy or tensors)."""
    count, sum, lowest = (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in (profile.count, profile.sum, profile.lowest))
    contig_bin, contig_genome = np.asarray(profile.contig_bin, dtype=np.int64), np.asarray(profile.contig_genome, dtype=np.int64)
    bin_length = int(profile.bin_length)
    if len(contig_bin) != len(contig_genome) + 1 or not (len(count) == len(sum) == len(lowest) == int(contig_bin[-1])):
        raise ValueError("the profile holds one entry per bin of the contigs")
    if len(contig_genome) and not 0 <= int(contig_genome.min()) <= int(contig_genome.max()) < len(names):
        raise ValueError("one name per reference genome")
    first_contig = np.searchsorted(contig_genome, np.arange(len(names)))       # the first contig of every genome
    with open(path, "w") as f:
        f.write("\t".join(PROFILE_COLUMNS) + "\n")
        for c, genome in enumerate(contig_genome.tolist()):
            for at in range(int(contig_bin[c]), int(contig_bin[c + 1])):
                n, start = int(count[at]), (at - int(contig_bin[c])) * bin_length
                values = (f"{int(sum[at]) / n / 2.0 ** 20:.6g}", f"{float(lowest[at]):.6g}") if n else ("NA", "NA")
                f.write(f"{names[genome]}\t{c - int(first_contig[genome])}\t{start}\t{start + bin_length}\t{n}\t{values[0]}\t{values[1]}\n")


REGION_COLUMNS = ("genome", "contig", "start", "end", "entries", "hits", "mean_identity")


def write_regions(path, names, regions, segment_genome, segment_contig, unit, offset=0):
    """The regions of a profile (`conservation.ReferenceProfile.regions`, `conservation.FragmentProfile.regions`) as a
    BED-like tab-separated table, one line per region in the order given under a header line naming the columns
    (`REGION_COLUMNS`).  ``segment_genome[s]`` and ``segment_contig[s]`` are the genome (an index into ``names``) and the
    contig's number inside it of segment ``s``; ``unit`` is the length of an entry in bases -- ``bin_length`` on the reference
    side, the fragment length on the query side --, so a region covers ``[offset + first * unit, offset + (first + length) *
    unit)`` of its contig, half open.  ``entries`` is the region's length in entries, ``hits`` the sum of their counts, and
    ``mean_identity`` ``sum / hits / 2**20``, ``NA`` where ``hits`` is 0 (a region of absence)."""
    if int(unit) < 1:
        raise ValueError("unit must be positive")
    if len(segment_genome) != len(segment_contig):
        raise ValueError("one genome and one contig number per segment")
    with open(path, "w") as f:
        f.write("\t".join(REGION_COLUMNS) + "\n")
        for r in regions:
            s, first, length, hits = int(r["segment"]), int(r["first"]), int(r["length"]), int(r["hits"])
            if not 0 <= s < len(segment_genome):
                raise ValueError("a region names a segment outside the segments given")
            start = int(offset) + first * int(unit)
            mean = f"{int(r['sum']) / hits / 2.0 ** 20:.6g}" if hits else "NA"
            f.write(f"{names[int(segment_genome[s])]}\t{int(segment_contig[s])}\t{start}\t{start + length * int(unit)}\t{length}\t{hits}\t{mean}\n")
