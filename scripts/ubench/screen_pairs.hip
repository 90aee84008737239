// Micro-benchmark (gfx950): k_screen_pairs -- the PRODUCT kernel -- at 1, 2, 4 and 8 elements of A per lane and pass, on
// synthetic signatures: n genomes (default 4000) at s (default 1000) in families of ten, every member holding s of a
// family pool of 1.3 s ascending hashes, triangular, at the Jaccard cut-off of distance 0.1 at k = 16.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o screen_pairs screen_pairs.hip && ./screen_pairs [n] [s] >> profiles/screen_pair_kernel.txt
//
// The variants run in turn, five rounds after a warm-up round, timed by device events around the one launch; the masks of
// all variants must be equal.  The bound printed next to the times counts the LDS reads of the one-element form exactly
// as scripts/time_screen.py does (a read of A, one per search step and one of B per pass over 64 elements, until a rank
// reaches s), at 2 LDS cycles per ds_read_b32 wave instruction, over all CUs at the clock the device reports.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../pyfastani_amd/csrc/fa_screen.hip.h"

using namespace fa;
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

template <int E>
static float run(const ScreenArgs &a, dim3 grid, size_t lds, hipEvent_t e0, hipEvent_t e1) {
  (void)hipMemset(a.mask, 0, (size_t)a.n_words * sizeof(unsigned long long));
  (void)hipEventRecord(e0, nullptr);
  hipLaunchKernelGGL(k_screen_pairs<E>, grid, dim3(SCR_THREADS), lds, nullptr, a);
  (void)hipEventRecord(e1, nullptr);
  (void)hipEventSynchronize(e1);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  return ms;
}

int main(int argc, char **argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 4000, s = argc > 2 ? atoi(argv[2]) : 1000, FAMILY = 10;
  if (n < 2 || s < 1 || s > SCR_MAX_S) { printf("usage: screen_pairs [n >= 2] [1 <= s <= 4096]\n"); return 1; }
  hipDeviceProp_t prop; CHECK(hipGetDeviceProperties(&prop, 0));
  // ---- synthetic signatures ----
  std::mt19937 rng(12345);
  const int pool_size = s + (3 * s + 9) / 10;
  std::vector<uint32_t> sig((size_t)n * s), pool(pool_size);
  std::vector<int32_t> count(n, s);
  std::vector<int> pick(pool_size);
  const uint32_t max_gap = std::max(2u, (uint32_t)(0x20000000u / (uint32_t)pool_size));        // a pool fills the lowest eighth
  for (int g = 0; g < n; g++) {
    if (g % FAMILY == 0) {
      uint32_t v = 0;
      for (int i = 0; i < pool_size; i++) { v += 1 + rng() % max_gap; pool[i] = v; }
    }
    for (int i = 0; i < pool_size; i++) pick[i] = i;
    std::shuffle(pick.begin(), pick.end(), rng);
    std::sort(pick.begin(), pick.begin() + s);
    for (int i = 0; i < s; i++) sig[(size_t)g * s + i] = pool[pick[i]];
  }
  // ---- the LDS reads of the one-element form, on a sample of pairs ----
  double reads = 0;
  const int sample = 2000;
  for (int k = 0; k < sample; k++) {
    const int ga = (int)(rng() % n), gb = (int)(rng() % n);
    const uint32_t *A = sig.data() + (size_t)ga * s, *B = sig.data() + (size_t)gb * s;
    int steps = 0;
    while ((1 << steps) <= s) steps++;
    int matches = 0, passes = 0;
    for (int base = 0; base < s; base += 64) {
      passes++;
      const int lo = (int)(std::lower_bound(B, B + s, A[base]) - B);
      if (base + lo - matches >= s) break;
      for (int i = base; i < std::min(s, base + 64); i++) matches += std::binary_search(B, B + s, A[i]) ? 1 : 0;
    }
    reads += (double)passes * (steps + 2);
  }
  reads /= sample;
  // ---- device ----
  uint32_t *d_sig; int32_t *d_count; TableStatus *d_status;
  ScreenArgs a{};
  a.n_a = a.n_b = n; a.s = s; a.triangular = 1; a.jn = 117736; a.jd = 1 << 20;
  a.tile = screen_tile(s);
  a.tile_shift = 31 - __builtin_clz((unsigned)a.tile);
  a.tiles_a = (n + a.tile - 1) / a.tile;
  a.words_per_row = (n + 63) / 64;
  a.n_words = (int64_t)n * a.words_per_row;
  CHECK(hipMalloc(&d_sig, sig.size() * 4));
  CHECK(hipMalloc(&d_count, (size_t)n * 4));
  CHECK(hipMalloc(&d_status, sizeof(TableStatus)));
  CHECK(hipMalloc(&a.mask, (size_t)a.n_words * 8));
  CHECK(hipMemcpy(d_sig, sig.data(), sig.size() * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_count, count.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  CHECK(hipMemset(d_status, 0, sizeof(TableStatus)));
  a.sig_a = a.sig_b = d_sig; a.count_a = a.count_b = d_count; a.status = d_status;
  const dim3 grid((unsigned)a.tiles_a, (unsigned)std::min(a.tiles_a, 65535));
  const size_t lds = (size_t)2 * a.tile * screen_stride(s) * sizeof(uint32_t);
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  const int variants[4] = {1, 2, 4, 8}, ROUNDS = 6;
  std::vector<float> ms[4];
  std::vector<unsigned long long> first((size_t)a.n_words), other((size_t)a.n_words);
  bool equal = true;
  for (int round = 0; round < ROUNDS; round++) {                     // (round 0 warms up)
    for (int v = 0; v < 4; v++) {
      float t = 0;
      switch (variants[v]) {
        case 1: t = run<1>(a, grid, lds, e0, e1); break;
        case 2: t = run<2>(a, grid, lds, e0, e1); break;
        case 4: t = run<4>(a, grid, lds, e0, e1); break;
        default: t = run<8>(a, grid, lds, e0, e1); break;
      }
      CHECK(hipGetLastError());
      if (round) ms[v].push_back(t);
      else {
        CHECK(hipMemcpy((v ? other : first).data(), a.mask, (size_t)a.n_words * 8, hipMemcpyDeviceToHost));
        if (v) equal = equal && other == first;
      }
    }
  }
  TableStatus status;
  CHECK(hipMemcpy(&status, d_status, sizeof status, hipMemcpyDeviceToHost));
  size_t kept = 0;
  for (unsigned long long w : first) kept += (size_t)__builtin_popcountll(w);
  const double pairs = (double)n * (n - 1) / 2, clock_hz = (double)prop.clockRate * 1e3;
  const double bound_ms = pairs * reads * 2.0 / ((double)prop.multiProcessorCount * clock_hz) * 1e3;
  printf("k_screen_pairs  %s  n %d  s %d  tile %d  pairs %.0f  kept %zu  flags %u  masks equal %s\n", prop.gcnArchName, n, s, a.tile, pairs,
         kept, status.flags, equal ? "yes" : "NO");
  printf("  LDS read bound (one-element form, conflict-free): %.1f ds_read_b32 per pair, %d CUs at %.2f GHz: %.3f ms\n", reads,
         prop.multiProcessorCount, clock_hz * 1e-9, bound_ms);
  for (int v = 0; v < 4; v++) {
    std::sort(ms[v].begin(), ms[v].end());
    printf("  %d per lane: median %.3f ms (min %.3f, max %.3f)  %.2f of the bound\n", variants[v], ms[v][ms[v].size() / 2], ms[v].front(),
           ms[v].back(), bound_ms / ms[v][ms[v].size() / 2]);
  }
  return equal && !status.flags ? 0 : 1;
}
