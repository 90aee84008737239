// fa_order.h -- the caller's order of preference over the genomes (fa_table_representatives) checked and inverted: plain C++,
// no HIP (scripts/host_sanitize/order.cpp checks it on the CPU).
//
// `order` lists the genome numbers 0 .. n-1, the most preferred first; a null pointer stands for genome-number order.  The
// selection works on the inverse, pos[g] = the place of g in `order`.  Anything that is not a permutation -- a value outside
// [0, n), a value that occurs twice (and therefore one that is missing) -- is refused before any device work.
#pragma once

#include <cstdint>
#include <vector>

namespace fa {

// pos [n] from order [n]; false when `order` is no permutation of 0 .. n-1 (pos then holds nothing of use)
inline bool order_positions(const int32_t *order, int32_t n, std::vector<int32_t> &pos) {
  pos.assign((size_t)(n > 0 ? n : 0), -1);
  for (int32_t i = 0; i < n; i++) {
    const int32_t g = order ? order[i] : i;
    if ((uint32_t)g >= (uint32_t)n || pos[(size_t)g] >= 0) return false;
    pos[(size_t)g] = i;
  }
  return true;
}

}  // namespace fa
