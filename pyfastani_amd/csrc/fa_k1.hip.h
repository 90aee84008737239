// fa_k1.hip.h -- the launcher of K1, the winnowed-minimizer kernels (k_sketch_tiles, fa_sketch.hip.h; k_sketch_fast,
// fa_sketch_fast.hip.h; k_query_fused, fa_map.hip.h), shared by reference sketching and the query pass, and the staging
// buffers it fills.  Host side of the one translation unit fa_engine.hip.
#pragma once

#include <algorithm>

#include "fa_common.h"
#include "fa_knobs.h"
#include "fa_map.hip.h"
#include "fa_sketch.hip.h"
#include "fa_sketch_fast.hip.h"

using namespace fa;

// launches `kernel` with `lds` bytes of dynamic LDS; above 64 KB the kernel has to be allowed them first
template <typename Kernel, typename... Args>
static void launch_lds(Kernel kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &...args) {
  if (lds > 64 * 1024) FA_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
}

// ------------------------------------------------------------------------------------------------------------
// K1 launcher shared by the reference and the query side
// ------------------------------------------------------------------------------------------------------------
struct SketchWork {
  DevBuf<Tile> tiles;
  DevBuf<uint32_t> stage_hash;
  DevBuf<int32_t> stage_wpos;
  DevBuf<int32_t> tile_count;   // ntiles + 1
  DevBuf<int32_t> tile_off;     // ntiles + 1
  DevBuf<unsigned char> cub_temp;
  // room for the staged records and the counts of `ntiles` tiles
  void reserve(size_t ntiles) { stage_hash.ensure(ntiles * TILE); stage_wpos.ensure(ntiles * TILE); tile_count.ensure(ntiles + 1); }
};

// `clear` (a query pass): ranges zeroed by extra workgroups of the first launch, beside the hashing
// `fuse` (a query pass, F fragments): K1 and the per-fragment sketch in one launch (k_query_fused) where the pass qualifies
// -- returns true then, and the caller skips k_query_sketch
static bool launch_sketch_tiles(const fa_params &P, const StoreView &store, const Tile *d_tiles, int ntiles, uint32_t *stage_hash,
                                int32_t *stage_wpos, int32_t *tile_count, hipStream_t st, const ClearArgs *clear = nullptr,
                                const QuerySketchArgs *fuse = nullptr, int64_t F = 0) {
  if (ntiles <= 0) {
    if (clear && clear->count) hipLaunchKernelGGL(k_clear, dim3(256), dim3(256), 0, st, *clear);
    return false;
  }
  SketchArgs a;
  a.ntiles = ntiles;
  a.clear.count = 0; a.clear.stamp = nullptr;
  int extra = 0;
  if (clear && clear->count) {
    a.clear = *clear;
    uint64_t most = 0;
    for (int i = 0; i < clear->count; i++) most = std::max(most, clear->n16[i]);
    extra = (int)std::min<uint64_t>(512, std::max<uint64_t>(1, (most + SK_THREADS * 8 - 1) / (SK_THREADS * 8)));
  }
  a.tiles = d_tiles;
  a.packed = store.packed; a.bytes = store.bytes; a.exc_pos = store.exc_pos; a.exc_val = store.exc_val;
  a.stage_hash = stage_hash; a.stage_wpos = stage_wpos; a.tile_count = tile_count;
  a.k = P.kmer_size; a.w = P.window_size; a.levels = floor_log2(P.window_size);
  a.protein = P.alphabet_size != 4;
  a.npos_cap = TILE + 2 * P.window_size - 2;
  // FA_K1_GENERAL=1: every tile through the 64-bit form of the window minimum (tests compare the two)
  const bool k1_general = knob::k1_general() != 0;
  a.fast = (!k1_general && P.window_size >= 3 && P.window_size <= 1000) ? 1 : 0;   // (three padded arrays in the LDS of two key arrays)
  const SketchLayout layout = sketch_layout(P.kmer_size, P.window_size);
  const size_t lds = layout.total;
  a.code_words = (int32_t)(layout.image / 4);
  // (`bytes` of dynamic LDS: the general forms' `lds`, which may need the 64 KB attribute; the fast forms' 13 KB never do, so
  // their launches make no runtime call besides the launch)
  auto launch = [&](auto kernel, size_t bytes) {
    launch_lds(kernel, dim3(ntiles + extra), dim3(SK_THREADS), bytes, st, a);
    extra = 0; a.clear.count = 0; a.clear.stamp = nullptr;          // (only the first launch zeroes)
  };
  // plain-ACGT tiles from the 2-bit image; protein tiles and tiles with other bytes through the byte image
  if (!a.protein && !k1_general && P.window_size >= SKF_MIN_W && P.window_size <= SKF_MAX_W) {
    // the hot form (fa_sketch_fast.hip.h): 13 KB of LDS, eight workgroups per CU; k = 14 / 16 / 21 hash from the premix tables
    const size_t flds = skf_layout(P.kmer_size, P.window_size).total;
    // The (k, w) cells of the default identity cut-off over the usual fragment lengths -- BASELINE config 5's grid: k in
    // {14, 16, 21} x fragment in {1000, 3000, 5000}, windows from recommendedWindowSize -- are built with BOTH parameters at
    // compile time (the window loop unrolled, 42 registers instead of 61 in k_sketch_fast); any other window takes the
    // run-time form of its k.
#define FA_KW_CELLS(X) X(14, 12) X(14, 37) X(14, 50) X(16, 13) X(16, 24) X(16, 40) X(21, 15) X(21, 25)
    // fused with the per-fragment sketch (k_query_fused, one of those cells): fragments whose records fit QF_CAP with room to
    // spare (a denser one voids the pass).  Tiles that touch a byte outside ACGT are sketched by k_sketch_tiles<0, true> into the
    // staging arrays FIRST (a launch whose other workgroups exit at once, and which carries the zeroing workgroups of the pass);
    // the fused kernel takes their records from there.  The run-time-w forms of the fused kernel do not fit the registers of seven waves per
    // SIMD -- a few words would go to scratch memory, which the runtime then keeps per stream for good -- and are not built.
    const bool fuse_on = knob::query_fused() != 0;
    const bool may_fuse = fuse && fuse_on && (int64_t)5 * P.fragment_length / (P.window_size + 1) <= QF_CAP;
    bool served = false;
#define FA_TRY_CELL(K, W)                                                                                                        \
    if (!served && P.kmer_size == K && P.window_size == W) {                                                                      \
      served = true;                                                                                                              \
      if (may_fuse) {                                                                                                             \
        QuerySketchArgs qa = *fuse;                                                                                               \
        qa.exc_tiles = store.n_exc > 0 ? 1 : 0;                                                                                   \
        if (store.n_exc > 0) launch(k_sketch_tiles<0, true>, lds);                                                                \
        const size_t qlds = flds + (size_t)QF_CAP * 4;                                                                            \
        hipLaunchKernelGGL((k_query_fused<K, W>), dim3((unsigned)F + extra), dim3(SK_THREADS), qlds, st, a, qa, (int)F);            \
        FA_HIP(hipGetLastError());                                                                                                \
        return true;                                                                                                              \
      }                                                                                                                           \
      launch(k_sketch_fast<K, W>, flds);                                                                                          \
    }
    FA_KW_CELLS(FA_TRY_CELL)
#undef FA_TRY_CELL
#undef FA_KW_CELLS
    if (served) {}
    else if (P.kmer_size == 16) launch(k_sketch_fast<16, 0>, flds);
    else if (P.kmer_size == 14) launch(k_sketch_fast<14, 0>, flds);
    else if (P.kmer_size == 21) launch(k_sketch_fast<21, 0>, flds);
    else launch(k_sketch_fast<0, 0>, flds);
  } else if (!a.protein) { if (P.kmer_size == 16) launch(k_sketch_tiles<16, false>, lds); else launch(k_sketch_tiles<0, false>, lds); }
  if (a.protein || store.n_exc > 0) launch(k_sketch_tiles<0, true>, lds);
  FA_HIP(hipGetLastError());
  return false;
}
