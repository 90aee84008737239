// fa_knobs.h -- every environment variable libfastani_hip.so reads, in ONE table: its name, how its value is parsed, its
// default, when it is read, and what it does.  Plain C++ (no HIP, standard headers only): the engine and the host-side headers
// include it, scripts/host_sanitize/knobs.cpp pins the parsing and the read times, tests/test_knobs_host.py holds the names
// against the README's table and against every name the tests and scripts set.  (LOCAL_WORLD_SIZE, the launcher's variable
// behind the default of FA_HOST_THREADS, is the one variable read outside this file: fa_host.h.)
//
// A row is X(identifier, "NAME", kind, default, when, "what it does") and becomes the inline function fa::knob::identifier().
//
// kind -- the parsers, unchanged since they were env_set / env_num / env_u64 in fa_engine.hip:
//   FLAG             bool      set to anything, the empty string included
//   NUM              double    atof of the value ("" and "abc" are 0.0); the default column is what an UNSET variable gives --
//                              UNSET itself (a NaN, knob::unset(v)) where the call site must tell "not set" from every number,
//                              INF where the call site clamps against a constant of a kernel header (the one string that now
//                              reads differently: "nan" for FA_TRACE / FA_POOL_MAX_GB counts as not set)
//   COUNT            uint64_t  atoll of the value where that is positive ("12abc" is 12, "1e3" is 1), else the default ("0", "-5",
//                              "abc", ""); 0 as default = "not given", the call site computes or validates
//   COUNT_IN(lo, hi)           a COUNT clamped into [lo, hi]
//   COUNT_UP(m)                a COUNT rounded up to a multiple of m
//   TEXT             string    the value as it stands
// when:
//   ONCE  read at the first call of THIS accessor and cached for the life of the process (a function-local static): tests that
//         force such a knob start a child process
//   LIVE  the environment is consulted on every call.  FA_QF_CAP, FA_NO_PACKED_GEO and FA_EVENTS_CAP_MAX are read by every query
//         pass (once per part), FA_GPOS_BITS / FA_LINK_BLOCK_BITS / FA_FREQ_OVER_CAP by every index build (the last also by
//         fa_sketch_frequency, through the same function), FA_TRACE wherever a traced stage starts; FA_SMAX_INIT /
//         FA_LOCI_CAP_MIN / FA_EVENTS_CAP_MIN at the first query of every mapper and
//         FA_MAP_STAGE_MB when a mapper is built (call sites that run once per object)
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <limits>
#include <string>

#define FA_KNOBS(X)                                                                                                                \
  /* ---- forms of the query pass (each bit-exact with the default) ---- */                                                        \
  X(query_fused, "FA_QUERY_FUSED", NUM, 1, ONCE, "0: grid-cell query passes through k_sketch_fast + k_query_sketch, not k_query_fused") \
  X(query_zero_copy, "FA_QUERY_ZERO_COPY", NUM, 1, ONCE, "0: the one-query call copies its packed query to HBM instead of sketching from the pinned image") \
  X(k1_general, "FA_K1_GENERAL", NUM, 0, ONCE, "1: every tile through k_sketch_tiles and its 64-bit window minimum")               \
  X(k1_tile, "FA_K1_TILE", COUNT, 0, ONCE, "positions per reference tile (a multiple of 4 in [256, TILE], else ignored); 1024: full tiles") \
  X(l1_block_sort, "FA_L1_BLOCK_SORT", NUM, 1, ONCE, "0: k_l1 merges the position lists instead of sorting the hits block-wise")   \
  X(l1_big, "FA_L1_BIG", NUM, 1, ONCE, "0: oversized fragments stay on the HBM sort instead of the chunked k_l1_big")               \
  X(l1_near, "FA_L1_NEAR", NUM, -1, ONCE, "0 / 1: k_l1 never / always skips the coordinate fetch of hits that cannot end a candidate") \
  X(l1_prefilter, "FA_L1_PREFILTER", NUM, -1, ONCE, "0 / 1: k_l1 never / always drops hits that cannot belong to a candidate before its block sort") \
  X(l1_thin_small, "FA_L1_THIN_SMALL", NUM, -1.0, ONCE, "share below which the small size class of k_l1 gets no launch (< 0: the policy's)") \
  X(l1_thin_mid, "FA_L1_THIN_MID", NUM, 0.05, ONCE, "share below which the middle size class of k_l1 gets no launch")              \
  X(l2_scan_order, "FA_L2_SCAN_ORDER", NUM, -1, ONCE, "0 / 1: k_l2_scan never / always takes its loci sorted by stream length")    \
  X(frag_order, "FA_FRAG_ORDER", NUM, 1, ONCE, "0: query-major workgroup order of k_l2_events in passes of several genomes")       \
  X(frag_order_one, "FA_FRAG_ORDER_ONE", NUM, 1, ONCE, "0: identity workgroup order of k_l2_events in a pass of one genome")       \
  X(no_packed_geo, "FA_NO_PACKED_GEO", FLAG, false, LIVE, "k_l2_events reads the unpacked index arrays")                           \
  X(rows_emit_max, "FA_ROWS_EMIT_MAX", COUNT_IN(1, 16384), 512, ONCE, "pairs of a pass up to which the last workgroup of k_cgi_rows forms the rows") \
  X(pass_fragments, "FA_PASS_FRAGMENTS", COUNT, 48 * 1024, ONCE, "fragments per device pass")                                      \
  X(spin_us, "FA_SPIN_US", COUNT, 20000, ONCE, "microseconds a call polls for a pass's status before it sleeps on the stream")     \
  X(map_stage_mb, "FA_MAP_STAGE_MB", COUNT, 64, LIVE, "megabytes per stage buffer of the streamed mapping output")                 \
  /* ---- hooks of the test suite: speculation retries, part splitting, the rare roads of the index build ---- */                  \
  X(qf_cap, "FA_QF_CAP", NUM, INF, LIVE, "records of a fragment k_query_fused holds (clamped to [0, QF_CAP])")                     \
  X(smax_init, "FA_SMAX_INIT", COUNT, 256, LIVE, "a mapper's first guess of the largest query sketch")                             \
  X(loci_cap_min, "FA_LOCI_CAP_MIN", COUNT, 1u << 18, LIVE, "a mapper's first room for loci")                                      \
  X(events_cap_min, "FA_EVENTS_CAP_MIN", COUNT, 1u << 26, LIVE, "a mapper's first room for slide events")                          \
  X(events_cap_max, "FA_EVENTS_CAP_MAX", COUNT, (1ULL << 32) - 64, LIVE, "most slide events one part of a pass may hold")          \
  X(gpos_bits, "FA_GPOS_BITS", COUNT_IN(12, 32), 32, LIVE, "bits of the low word of a record's global coordinate")                 \
  X(link_block_bits, "FA_LINK_BLOCK_BITS", COUNT_IN(2, 20), 10, LIVE, "log2 of the records per block of k_link_duplicates")        \
  X(freq_over_cap, "FA_FREQ_OVER_CAP", COUNT_IN(1, 1u << 16), 1u << 16, LIVE, "long position lists the frequency histogram keeps verbatim") \
  /* ---- diagnostics, to stderr ---- */                                                                                           \
  X(trace, "FA_TRACE", NUM, UNSET, LIVE, "set: wall-clock split of sketching, index build, upload, FASTA reading; >= 2: every stage as it ends") \
  X(debug_sync, "FA_DEBUG_SYNC", FLAG, false, ONCE, "synchronise after every stage of a query pass and name it")                   \
  X(debug_l1, "FA_DEBUG_L1", FLAG, false, ONCE, "the size classes and launches of k_l1, per part")                                 \
  X(l1_stats, "FA_L1_STATS", NUM, 0, ONCE, "1: which road the fragments of k_l1 took and the ticks of its phases (one workgroup in 64)") \
  /* ---- the host side ---- */                                                                                                    \
  X(host_threads, "FA_HOST_THREADS", COUNT, 0, ONCE, "host packer threads (not given: hardware threads / LOCAL_WORLD_SIZE, at most 128)") \
  X(pool_max_gb, "FA_POOL_MAX_GB", NUM, UNSET, ONCE, "GB of device memory kept for reuse (not given: 30 % of the device, at most 96)") \
  X(no_avx2, "FA_NO_AVX2", FLAG, false, ONCE, "table-driven host packer")                                                          \
  X(pack_chunk, "FA_PACK_CHUNK", COUNT_UP(64), 0, ONCE, "bases per packing task (not given: 2^18 with AVX2, else 2^16)")           \
  X(fasta_io, "FA_FASTA_IO", TEXT, "", ONCE, "mmap: the FASTA reader maps files instead of read()ing them")                        \
  X(fasta_threads, "FA_FASTA_THREADS", COUNT, 24, ONCE, "pool workers that read FASTA files")

namespace fa {
namespace knob {

constexpr double UNSET = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();
inline bool unset(double v) { return v != v; }

namespace detail {
inline bool flag(const char *name) { return getenv(name) != nullptr; }
inline double num(const char *name, double unset) {
  const char *e = getenv(name);
  return e ? atof(e) : unset;
}
inline uint64_t count(const char *name, uint64_t dflt) {
  const char *e = getenv(name);
  const long long x = e ? atoll(e) : 0;
  return x > 0 ? (uint64_t)x : dflt;
}
template <uint64_t LO, uint64_t HI>
inline uint64_t count_in(const char *name, uint64_t dflt) { return std::min<uint64_t>(HI, std::max<uint64_t>(LO, count(name, dflt))); }
template <uint64_t M>
inline uint64_t count_up(const char *name, uint64_t dflt) { return (count(name, dflt) + M - 1) / M * M; }
inline std::string text(const char *name, const char *dflt) {
  const char *e = getenv(name);
  return e ? e : dflt;
}
}  // namespace detail

#define FA_KNOB_TYPE_FLAG bool
#define FA_KNOB_TYPE_NUM double
#define FA_KNOB_TYPE_COUNT uint64_t
#define FA_KNOB_TYPE_COUNT_IN(lo, hi) uint64_t
#define FA_KNOB_TYPE_COUNT_UP(m) uint64_t
#define FA_KNOB_TYPE_TEXT std::string
#define FA_KNOB_READ_FLAG(name, dflt) detail::flag(name)
#define FA_KNOB_READ_NUM(name, dflt) detail::num(name, dflt)
#define FA_KNOB_READ_COUNT(name, dflt) detail::count(name, dflt)
#define FA_KNOB_READ_COUNT_IN(lo, hi) detail::count_in<lo, hi>
#define FA_KNOB_READ_COUNT_UP(m) detail::count_up<m>
#define FA_KNOB_READ_TEXT(name, dflt) detail::text(name, dflt)
#define FA_KNOB_ONCE static const
#define FA_KNOB_LIVE const
#define FA_KNOB_ACCESSOR(id, name, kind, dflt, when, what) \
  inline FA_KNOB_TYPE_##kind id() { FA_KNOB_##when FA_KNOB_TYPE_##kind v = FA_KNOB_READ_##kind(name, dflt); return v; }
FA_KNOBS(FA_KNOB_ACCESSOR)
#undef FA_KNOB_ACCESSOR
#undef FA_KNOB_ONCE
#undef FA_KNOB_LIVE
#undef FA_KNOB_TYPE_FLAG
#undef FA_KNOB_TYPE_NUM
#undef FA_KNOB_TYPE_COUNT
#undef FA_KNOB_TYPE_COUNT_IN
#undef FA_KNOB_TYPE_COUNT_UP
#undef FA_KNOB_TYPE_TEXT
#undef FA_KNOB_READ_FLAG
#undef FA_KNOB_READ_NUM
#undef FA_KNOB_READ_COUNT
#undef FA_KNOB_READ_COUNT_IN
#undef FA_KNOB_READ_COUNT_UP
#undef FA_KNOB_READ_TEXT

}  // namespace knob
}  // namespace fa
