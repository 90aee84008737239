// fa_error.h -- the error type and argument checks of libfastani_hip: plain C++, no HIP (the host-only pieces -- packer,
// FASTA reader, statistics, workspace leases -- build from this alone, which is what scripts/host_sanitize.sh compiles).
#pragma once

#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/fastani_hip.h"

namespace fa {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &msg) : std::runtime_error(msg), code(c) {}
};

#define FA_REQUIRE(cond, code, msg) do { if (!(cond)) throw ::fa::Error((code), (msg)); } while (0)

inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
// bits needed to write v (0 for 0): the one way to size a radix-sort key.  id_bits(n) = those of the largest of n ids, 1 at least
inline unsigned bit_width_u64(unsigned long long v) { return v ? 64u - (unsigned)__builtin_clzll(v) : 0u; }
inline unsigned id_bits(int64_t n) { return n > 1 ? bit_width_u64((unsigned long long)(n - 1)) : 1u; }
inline uint32_t next_pow2(uint32_t v) {
  uint32_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

}  // namespace fa
