"""MI355X-native FastANI fragment-mapping engine with pyfastani's Python surface.

Drop-in for the path ``Sketch`` -> ``add_draft``/``add_genome`` -> ``index`` -> ``Mapper.query_draft``/
``query_genome`` of `pyfastani <https://github.com/althonos/pyfastani>`_ (reference:
``src/pyfastani/__init__.py:1-27``).  The classes live in the Cython module ``pyfastani_amd._fastani`` (the reference's
``_fastani.pyx`` re-based on ``fastani_hip.pxd``); all compute runs in hand-written HIP kernels for
gfx950 behind the C ABI of ``include/fastani_hip.h``.  There is no CPU fallback, and importing the package needs neither
PyTorch nor numpy (``pyfastani_amd.sharding``, the multi-GPU layer, imports torch when it is used).

Beyond the reference's surface: resident query batches (``Mapper.upload_genomes`` -> `GenomeBatch`), FASTA ingest, and the
fragment mappings behind the hits -- ``Mapper.query_draft_mappings`` / ``query_genome_mappings`` and
``GenomeBatch.query_mappings`` return them as ``pyfastani_amd._batch.MAPPING_DTYPE`` records (numpy),
``GenomeBatch.iter_mappings`` yields them range by range for tables that should not stay in memory, and
``pyfastani_amd.outputs`` places them on the query's contigs and writes them as a table.  `Rules` selects, per mapper
(``Sketch(rules=...)``, ``Mapper.rules``), among the readings of three rules the reference's sources leave open.
"""
try:
    from ._fastani import (
        MAX_KMER_SIZE,
        GenomeBatch,
        Hit,
        Mapper,
        MinimizerIndex,
        MinimizerInfo,
        PackedGenomes,
        Minimizers,
        Position,
        Rules,
        Sketch,
        device_count,
        device_trim,
        pass_threshold,
        set_device,
    )
except ImportError as exc:  # the compiled binding or libfastani_hip.so is missing: there is nothing to fall back to
    raise ImportError(
        "pyfastani_amd needs its compiled binding (pyfastani_amd/_fastani*.so) and pyfastani_amd/lib/libfastani_hip.so: "
        "build them with `python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950 + cython). "
        f"There is no CPU fallback.  ({exc})"
    ) from exc

__all__ = [
    "MAX_KMER_SIZE", "Hit", "Mapper", "MinimizerIndex", "MinimizerInfo", "Minimizers", "Position", "Rules", "Sketch",
    "GenomeBatch", "PackedGenomes", "device_count", "device_trim", "pass_threshold", "set_device",
]
__version__ = "0.2.0"
