// The order check of fa_table_representatives (pyfastani_amd/csrc/fa_order.h) against a brute-force model, on the CPU: build
// with  g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all order.cpp  and run.
//
// For every n 0..40: the null order and random permutations are accepted and pos is their inverse; a permutation with one
// entry replaced by n, -1, INT32_MIN, INT32_MAX or another entry's value is refused, wherever the entry lies.  The arrays
// have exactly n entries, so under ASan a read or write beyond them is a finding of its own.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "../../pyfastani_amd/csrc/fa_order.h"

static int failures = 0;
#define CHECK(cond, ...) \
  do { if (!(cond)) { if (failures++ < 20) { fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int main() {
  long accepted = 0, refused = 0;
  std::vector<int32_t> pos;
  for (int32_t n = 0; n <= 40; n++) {
    CHECK(fa::order_positions(nullptr, n, pos) && (int32_t)pos.size() == n, "null order, n %d", n);
    for (int32_t g = 0; g < n; g++) CHECK(pos[(size_t)g] == g, "null order: pos[%d] = %d", g, pos[(size_t)g]);
    for (int trial = 0; trial < 20; trial++) {
      std::vector<int32_t> order((size_t)n);
      std::iota(order.begin(), order.end(), 0);
      for (int32_t i = n - 1; i > 0; i--) std::swap(order[(size_t)i], order[(size_t)(rnd() % (uint32_t)(i + 1))]);
      CHECK(fa::order_positions(order.data(), n, pos) && (int32_t)pos.size() == n, "a permutation of %d is refused", n);
      for (int32_t i = 0; i < n; i++) CHECK(pos[(size_t)order[(size_t)i]] == i, "pos is not the inverse at %d", i);
      accepted++;
      for (int32_t at = 0; at < n; at++) {
        const int32_t other = n > 1 ? order[(size_t)((at + 1 + (int32_t)(rnd() % (uint32_t)(n - 1))) % n)] : -1;
        for (int32_t bad : {n, (int32_t)-1, INT32_MIN, INT32_MAX, other}) {
          std::vector<int32_t> broken(order);
          broken[(size_t)at] = bad;
          CHECK(!fa::order_positions(broken.data(), n, pos), "n %d: entry %d replaced by %d is accepted", n, at, bad);
          refused++;
        }
      }
    }
  }
  printf("%ld orders accepted, %ld refused\n", accepted, refused);
  if (failures) { printf("%d checks FAILED\n", failures); return 1; }
  printf("all checks passed\n");
  return 0;
}
