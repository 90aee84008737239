"""Device side of the streamed-mapping tests (test_gpu_mapping_stream.py): maps one input set of hit_mappings.py at a list of
stage sizes inside ONE process and returns what the device gave, through every road the stream has -- the binding's
`query_mappings` / `iter_mappings`, and the C entry points with a counting sink, a null sink (count only) and the buffer
entry with no room.  Nothing here knows the expected values: the tests compare with hit_mappings.expected.

Run as a program (`python mapping_stream.py CASE OUT.npz S1,S2,... [fresh]`) it stores the sweep; the tests start it as a child
process where a case needs an environment variable set before HIP starts.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import hit_mappings as hm  # noqa: E402


def new_mapper(case):
    import pyfastani_amd as pf
    inp = hm.inputs(case)
    sk = pf.Sketch(**inp["params"])
    for i, contigs in enumerate(inp["refs"]):
        sk.add_draft(i, contigs)
    return sk.index()


class Sink:
    """A fa_mapping_sink that copies what it is given and notes the size of every call; `stop_at` = k: returns 1 on call k."""

    def __init__(self, stop_at=None):
        from pyfastani_amd import _lib
        from pyfastani_amd._batch import MAPPING_DTYPE
        self.sizes, self.parts, self.stop_at, self.dtype = [], [], stop_at, MAPPING_DTYPE
        self.cb = _lib.MAPPING_SINK(self._call)
        self.ptr = C.cast(self.cb, C.c_void_p)

    def _call(self, user, records, n):
        self.sizes.append(int(n))
        if self.stop_at is not None and len(self.sizes) == self.stop_at:
            return 1
        self.parts.append(np.frombuffer(C.string_at(records, int(n) * self.dtype.itemsize), dtype=self.dtype).copy())
        return 0

    def records(self):
        return np.concatenate(self.parts) if self.parts else np.zeros(0, self.dtype)


def stream_call(mapper, batch, first, count, sink_ptr):
    """fa_mapper_query_genomes_mappings_stream: (status code, rows, n_maps)"""
    from pyfastani_amd import _lib
    from pyfastani_amd._batch import ROW_DTYPE
    cap = max(1, count * max(1, len(mapper.names)))
    rows = np.zeros(cap, dtype=ROW_DTYPE)
    n_rows, n_maps = C.c_int64(0), C.c_int64(-1)
    code = _lib.lib.fa_mapper_query_genomes_mappings_stream(mapper._h, batch._h, first, count, rows.ctypes.data, cap, C.byref(n_rows), 0,
                                                            sink_ptr, None, C.byref(n_maps))
    return code, rows[: n_rows.value], n_maps.value


def buffer_call_without_room(mapper, batch, first, count):
    """fa_mapper_query_genomes_mappings with map_cap = 0 and a host destination: (status code, n_maps)"""
    from pyfastani_amd import _lib
    from pyfastani_amd._batch import ROW_DTYPE
    cap = max(1, count * max(1, len(mapper.names)))
    rows = np.zeros(cap, dtype=ROW_DTYPE)
    n_rows, n_maps = C.c_int64(0), C.c_int64(-1)
    code = _lib.lib.fa_mapper_query_genomes_mappings(mapper._h, batch._h, first, count, rows.ctypes.data, cap, C.byref(n_rows), 0,
                                                     None, 0, C.byref(n_maps), 0)
    return code, n_maps.value


def sweep(case, stages, fresh=False):
    """Every road at every stage size.  `fresh`: a mapper of its own per stage size whose FIRST query is `query_mappings`, so
    that the void parts a lowered capacity forces run with small windows on.  Keys: s{S}_{rows, maps, repeats, parts, memory,
    sink_code, sink_rows, sink_maps, sink_sizes, sink_count, sub_*, iter_ranges, iter_rows, iter_maps, null_code, null_count,
    old_code, old_count} and plain_rows."""
    import warnings
    from pyfastani_amd._batch import MAPPING_DTYPE, ROW_DTYPE
    inp = hm.inputs(case)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mapper = batch = None
        for S in stages:
            if fresh or mapper is None:
                mapper = new_mapper(case)
                batch = mapper.upload_genomes(inp["queries"])
            k = f"s{S}_"
            mapper.set_mapping_stage(S)
            out[k + "rows"], out[k + "maps"] = batch.query_mappings()
            out[k + "repeats"], out[k + "parts"] = hm.call_counters(mapper)
            out[k + "memory"] = np.array(mapper.mapping_memory(), dtype=np.int64)
            sink = Sink()
            out[k + "sink_code"], out[k + "sink_rows"], out[k + "sink_count"] = stream_call(mapper, batch, 0, len(batch), sink.ptr)
            out[k + "sink_maps"], out[k + "sink_sizes"] = sink.records(), np.array(sink.sizes, dtype=np.int64)
            if inp["sub"]:
                first, count = inp["sub"]
                out[k + "sub_rows"], out[k + "sub_maps"] = batch.query_mappings(first, count)
                sink = Sink()
                _, _, _ = stream_call(mapper, batch, first, count, sink.ptr)
                out[k + "sub_sink_maps"], out[k + "sub_sink_sizes"] = sink.records(), np.array(sink.sizes, dtype=np.int64)
            ranges, rows, maps = [], [np.zeros(0, ROW_DTYPE)], [np.zeros(0, MAPPING_DTYPE)]
            for lo, n, r, m in batch.iter_mappings():
                ranges.append((lo, n))
                rows.append(r)
                maps.append(m)
            out[k + "iter_ranges"] = np.array(ranges, dtype=np.int64).reshape(-1, 2)
            out[k + "iter_rows"], out[k + "iter_maps"] = np.concatenate(rows), np.concatenate(maps)
            out[k + "null_code"], _, out[k + "null_count"] = stream_call(mapper, batch, 0, len(batch), None)
            out[k + "old_code"], out[k + "old_count"] = buffer_call_without_room(mapper, batch, 0, len(batch))
        out["plain_rows"] = batch.query_rows()
    return out


if __name__ == "__main__":
    case, path, stages = sys.argv[1], sys.argv[2], [int(s) for s in sys.argv[3].split(",")]
    np.savez(path, **sweep(case, stages, fresh="fresh" in sys.argv[4:]))
    print("OK")
