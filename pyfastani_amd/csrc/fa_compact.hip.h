// fa_compact.hip.h -- the middle step of every ordered compaction of the library (count per chunk, scan the chunk counts,
// write): the mappings of a pass (fa_map.hip.h), the pairs and edges of a hit table (fa_table.hip.h), the pairs of a
// screen (fa_screen.hip.h) and the entries and records of its containment road (fa_contain.hip.h) count and write in their
// own kernels and share this scan.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace fa {

// exclusive 64-bit sum of the chunk counts by one workgroup (thread t owns a run of consecutive chunks) + the total.
// Launched as dim3(1), dim3(1024).
__global__ __launch_bounds__(1024) void k_chunk_scan(const int32_t *chunk_count, int64_t *chunk_off, int32_t n_chunks, int64_t *total) {
  __shared__ long long sh_wave[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int per = (n_chunks + 1023) / 1024;
  const int c0 = min(n_chunks, (int)threadIdx.x * per), c1 = min(n_chunks, c0 + per);
  long long mine = 0;
  for (int c = c0; c < c1; c++) mine += chunk_count[c];
  long long incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const long long v = __shfl_up(incl, d); if (lane >= d) incl += v; }
  if (lane == 63) sh_wave[wv] = incl;
  __syncthreads();
  long long off = incl - mine;
  for (int w = 0; w < wv; w++) off += sh_wave[w];
  for (int c = c0; c < c1; c++) { chunk_off[c] = off; off += chunk_count[c]; }
  if (threadIdx.x == 1023) *total = off;
}

}  // namespace fa
