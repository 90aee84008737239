// fa_mapstream.h -- the window arithmetic of the streamed mapping output: plain C++, no HIP
// (scripts/host_sanitize/mapstream.cpp checks it on the CPU).
//
// The records of a pass (fa_hit_mapping, k_map_count / k_chunk_scan / k_map_write in fa_map.hip.h) have places 0 .. total - 1 in
// (query, reference genome, bin) order.  They leave the device in windows of `stage` records: window w holds the places
// [w * stage, min(total, (w + 1) * stage)), written to the front of a stage buffer of fixed size.  k_map_write is launched once
// per window; a workgroup, which owns one chunk of consecutive bins and knows the place of its first record and their number,
// asks map_chunk_in_window whether any of them falls into the window before it loads a key.  fa_query.hip.h (QueryPass) owns the
// stage buffers and the launches; everything here is pure arithmetic.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define FA_MAPSTREAM_FN __host__ __device__ inline
#else
#define FA_MAPSTREAM_FN inline
#endif

namespace fa {

struct MapWindow { int64_t lo, hi; };   // places [lo, hi) of the pass

// windows of a pass of `total` records at `stage` (>= 1) records per window: none for an empty pass, no empty window
FA_MAPSTREAM_FN int64_t map_windows(int64_t total, int64_t stage) {
  return total <= 0 ? 0 : (total - 1) / stage + 1;          // (not (total + stage - 1) / stage: that sum may overflow)
}

// window w (0 <= w < map_windows(total, stage))
FA_MAPSTREAM_FN MapWindow map_window(int64_t total, int64_t stage, int64_t w) {
  MapWindow r;
  r.lo = w * stage;
  r.hi = total - r.lo < stage ? total : r.lo + stage;
  return r;
}

// whether a chunk whose `count` records have the places [off, off + count) holds a record of [lo, hi)
FA_MAPSTREAM_FN bool map_chunk_in_window(int64_t off, int64_t count, int64_t lo, int64_t hi) {
  return count > 0 && off < hi && off + count > lo;
}

}  // namespace fa
