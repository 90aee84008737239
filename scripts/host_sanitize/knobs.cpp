// The knob table of libfastani_hip (pyfastani_amd/csrc/fa_knobs.h) on the CPU: what every accessor makes of a value, and when
// it reads it.  Build with  g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all knobs.cpp  and run it
// twice: `knobs` and `knobs defaults` (a ONCE accessor answers one question per process).
//
// Every expected value below is written out by hand from the rules the header states -- none is computed with a copy of the
// parser.  LIVE accessors are walked through the whole list of strings of their kind (not set, "", "0", "-5", "abc", "12abc",
// "1e3", values at and beyond their clamps), each read following a setenv: a LIVE accessor that cached would fail at the second
// string.  ONCE accessors are set, read, set to something that parses differently, and read again: the first value stays.
// `defaults` reads every accessor with no FA_* variable set.  Values that overflow long long are not pinned.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <utility>

#include "../../pyfastani_amd/csrc/fa_knobs.h"

namespace knob = fa::knob;

static int failures = 0, checks = 0;
static std::string show(bool v) { return v ? "true" : "false"; }
static std::string show(double v) { return std::to_string(v); }
static std::string show(uint64_t v) { return std::to_string(v); }
static std::string show(const std::string &v) { return "\"" + v + "\""; }
static bool same(double a, double b) { return (std::isnan(a) && std::isnan(b)) || a == b; }
static bool same(bool a, bool b) { return a == b; }
static bool same(uint64_t a, uint64_t b) { return a == b; }
static bool same(const std::string &a, const std::string &b) { return a == b; }

static void put(const char *name, const char *value) {
  if (value) setenv(name, value, 1); else unsetenv(name);
}
template <typename T, typename W>
static void expect(const char *name, const char *value, T got, W want_) {
  const T want = (T)want_;
  checks++;
  if (same(got, want)) return;
  failures++;
  fprintf(stderr, "FAILED %s=%s: got %s, expected %s\n", name, value ? (std::string("\"") + value + "\"").c_str() : "(not set)", show(got).c_str(), show(want).c_str());
}
// a LIVE accessor follows the environment from call to call
template <typename T, typename W>
static void live(const char *name, T (*get)(), std::initializer_list<std::pair<const char *, W>> cases) {
  for (const auto &c : cases) { put(name, c.first); expect(name, c.first, get(), c.second); }
  unsetenv(name);
}
// a ONCE accessor keeps what it read first
template <typename T, typename W>
static void once(const char *name, T (*get)(), const char *first, W want, const char *then) {
  put(name, first);
  expect(name, first, get(), want);
  put(name, then);
  expect(name, first, get(), want);
  unsetenv(name);
}

static const double NaN = std::nan("");
typedef std::pair<const char *, double> N;
typedef std::pair<const char *, uint64_t> U;
typedef std::pair<const char *, bool> B;

static void values_and_disciplines() {
  // ---- LIVE: the whole list of its kind, each string behind another ----
  live<bool, bool>("FA_NO_PACKED_GEO", knob::no_packed_geo, {B{nullptr, false}, B{"", true}, B{"0", true}, B{nullptr, false}, B{"1", true}});
  live<double, double>("FA_TRACE", knob::trace, {N{nullptr, NaN}, N{"", 0.0}, N{"1", 1.0}, N{"2", 2.0}, N{"2.5", 2.5}, N{"abc", 0.0}, N{"-1", -1.0},
                                                  N{"1e3", 1000.0}, N{"12abc", 12.0}, N{nullptr, NaN}});
  live<double, double>("FA_QF_CAP", knob::qf_cap, {N{nullptr, INFINITY}, N{"100", 100.0}, N{"", 0.0}, N{"-3", -3.0}, N{"1e9", 1e9}, N{"0", 0.0}});
  live<uint64_t, uint64_t>("FA_SMAX_INIT", knob::smax_init, {U{nullptr, 256}, U{"8", 8}, U{"0", 256}, U{"-5", 256}, U{"abc", 256}, U{"", 256}, U{"12abc", 12},
                                                              U{"1e3", 1}, U{" 42", 42}, U{"9223372036854775807", 9223372036854775807ULL}, U{nullptr, 256}});
  live<uint64_t, uint64_t>("FA_LOCI_CAP_MIN", knob::loci_cap_min, {U{nullptr, 262144}, U{"7", 7}, U{"0", 262144}});
  live<uint64_t, uint64_t>("FA_EVENTS_CAP_MIN", knob::events_cap_min, {U{nullptr, 67108864}, U{"1000", 1000}, U{"-1", 67108864}});
  live<uint64_t, uint64_t>("FA_EVENTS_CAP_MAX", knob::events_cap_max, {U{nullptr, 4294967232ULL}, U{"9000", 9000}, U{"150000", 150000}, U{"", 4294967232ULL}});
  live<uint64_t, uint64_t>("FA_MAP_STAGE_MB", knob::map_stage_mb, {U{nullptr, 64}, U{"1", 1}, U{"abc", 64}, U{"3mb", 3}});
  // clamps: below, at, inside, at, above
  live<uint64_t, uint64_t>("FA_GPOS_BITS", knob::gpos_bits, {U{nullptr, 32}, U{"5", 12}, U{"12", 12}, U{"20", 20}, U{"32", 32}, U{"40", 32}, U{"0", 32}, U{"abc", 32}});
  live<uint64_t, uint64_t>("FA_LINK_BLOCK_BITS", knob::link_block_bits, {U{nullptr, 10}, U{"1", 2}, U{"2", 2}, U{"15", 15}, U{"20", 20}, U{"21", 20}, U{"", 10}, U{"-5", 10}});
  live<uint64_t, uint64_t>("FA_FREQ_OVER_CAP", knob::freq_over_cap, {U{nullptr, 65536}, U{"1", 1}, U{"65536", 65536}, U{"65537", 65536}, U{"100000", 65536}, U{"-1", 65536}});

  // ---- ONCE: (first string, its value, a second string that the accessor must not see) ----
  once<double, double>("FA_QUERY_FUSED", knob::query_fused, "", 0.0, "1");                 // NUM of "" is 0.0, not "unset"
  once<double, double>("FA_QUERY_ZERO_COPY", knob::query_zero_copy, "0", 0.0, nullptr);
  once<double, double>("FA_K1_GENERAL", knob::k1_general, "abc", 0.0, "1");
  once<double, double>("FA_L1_BLOCK_SORT", knob::l1_block_sort, nullptr, 1.0, "0");          // not set at the first read: the default for good
  once<double, double>("FA_L1_BIG", knob::l1_big, "0", 0.0, "1");
  once<double, double>("FA_L1_NEAR", knob::l1_near, "1", 1.0, "0");
  once<double, double>("FA_L1_PREFILTER", knob::l1_prefilter, nullptr, -1.0, "1");
  once<double, double>("FA_L1_THIN_SMALL", knob::l1_thin_small, "0.25", 0.25, "0.5");
  once<double, double>("FA_L1_THIN_MID", knob::l1_thin_mid, "12abc", 12.0, nullptr);
  once<double, double>("FA_L2_SCAN_ORDER", knob::l2_scan_order, "-1", -1.0, "1");
  once<double, double>("FA_FRAG_ORDER", knob::frag_order, "1e3", 1000.0, "0");
  once<double, double>("FA_FRAG_ORDER_ONE", knob::frag_order_one, " 2x", 2.0, "0");
  once<double, double>("FA_L1_STATS", knob::l1_stats, "1", 1.0, "0");
  once<double, double>("FA_POOL_MAX_GB", knob::pool_max_gb, "", 0.0, "8");                  // set to nothing: a pool of 0 GB, not the default
  once<uint64_t, uint64_t>("FA_PASS_FRAGMENTS", knob::pass_fragments, "12abc", 12, "16");
  once<uint64_t, uint64_t>("FA_SPIN_US", knob::spin_us, "1e3", 1, "5");
  once<uint64_t, uint64_t>("FA_ROWS_EMIT_MAX", knob::rows_emit_max, "99999", 16384, "3");    // clamped
  once<uint64_t, uint64_t>("FA_K1_TILE", knob::k1_tile, "-5", 0, "1024");
  once<uint64_t, uint64_t>("FA_HOST_THREADS", knob::host_threads, "0", 0, "8");
  once<uint64_t, uint64_t>("FA_FASTA_THREADS", knob::fasta_threads, "", 24, "3");
  once<uint64_t, uint64_t>("FA_PACK_CHUNK", knob::pack_chunk, "4097", 4160, "64");           // rounded up to a multiple of 64
  once<bool, bool>("FA_NO_AVX2", knob::no_avx2, "", true, nullptr);                          // FLAG set to "" is set
  once<bool, bool>("FA_DEBUG_SYNC", knob::debug_sync, nullptr, false, "1");
  once<bool, bool>("FA_DEBUG_L1", knob::debug_l1, "0", true, nullptr);
  once<std::string, std::string>("FA_FASTA_IO", knob::fasta_io, "mmap", "mmap", "read");
}

static void defaults() {
  expect("FA_QUERY_FUSED", nullptr, knob::query_fused(), 1.0);
  expect("FA_QUERY_ZERO_COPY", nullptr, knob::query_zero_copy(), 1.0);
  expect("FA_K1_GENERAL", nullptr, knob::k1_general(), 0.0);
  expect("FA_K1_TILE", nullptr, knob::k1_tile(), 0);
  expect("FA_L1_BLOCK_SORT", nullptr, knob::l1_block_sort(), 1.0);
  expect("FA_L1_BIG", nullptr, knob::l1_big(), 1.0);
  expect("FA_L1_NEAR", nullptr, knob::l1_near(), -1.0);
  expect("FA_L1_PREFILTER", nullptr, knob::l1_prefilter(), -1.0);
  expect("FA_L1_THIN_SMALL", nullptr, knob::l1_thin_small(), -1.0);
  expect("FA_L1_THIN_MID", nullptr, knob::l1_thin_mid(), 0.05);
  expect("FA_L2_SCAN_ORDER", nullptr, knob::l2_scan_order(), -1.0);
  expect("FA_FRAG_ORDER", nullptr, knob::frag_order(), 1.0);
  expect("FA_FRAG_ORDER_ONE", nullptr, knob::frag_order_one(), 1.0);
  expect("FA_NO_PACKED_GEO", nullptr, knob::no_packed_geo(), false);
  expect("FA_ROWS_EMIT_MAX", nullptr, knob::rows_emit_max(), 512);
  expect("FA_PASS_FRAGMENTS", nullptr, knob::pass_fragments(), 49152);
  expect("FA_SPIN_US", nullptr, knob::spin_us(), 20000);
  expect("FA_MAP_STAGE_MB", nullptr, knob::map_stage_mb(), 64);
  expect("FA_QF_CAP", nullptr, knob::qf_cap(), INFINITY);
  expect("FA_SMAX_INIT", nullptr, knob::smax_init(), 256);
  expect("FA_LOCI_CAP_MIN", nullptr, knob::loci_cap_min(), 262144);
  expect("FA_EVENTS_CAP_MIN", nullptr, knob::events_cap_min(), 67108864);
  expect("FA_EVENTS_CAP_MAX", nullptr, knob::events_cap_max(), 4294967232ULL);
  expect("FA_GPOS_BITS", nullptr, knob::gpos_bits(), 32);
  expect("FA_LINK_BLOCK_BITS", nullptr, knob::link_block_bits(), 10);
  expect("FA_FREQ_OVER_CAP", nullptr, knob::freq_over_cap(), 65536);
  expect("FA_TRACE", nullptr, knob::trace(), NaN);
  expect("FA_DEBUG_SYNC", nullptr, knob::debug_sync(), false);
  expect("FA_DEBUG_L1", nullptr, knob::debug_l1(), false);
  expect("FA_L1_STATS", nullptr, knob::l1_stats(), 0.0);
  expect("FA_HOST_THREADS", nullptr, knob::host_threads(), 0);
  expect("FA_POOL_MAX_GB", nullptr, knob::pool_max_gb(), NaN);
  expect("FA_NO_AVX2", nullptr, knob::no_avx2(), false);
  expect("FA_PACK_CHUNK", nullptr, knob::pack_chunk(), 0);
  expect("FA_FASTA_IO", nullptr, knob::fasta_io(), std::string());
  expect("FA_FASTA_THREADS", nullptr, knob::fasta_threads(), 24);
  if (!knob::unset(knob::trace()) || knob::unset(0.0) || knob::unset(INFINITY)) { failures++; fprintf(stderr, "FAILED knob::unset\n"); }
}

int main(int argc, char **argv) {
  // whatever the caller's environment holds: every variable of the table starts not set (the names, not the parsers, come from it)
  int rows = 0;
#define FA_UNSET(id, name, kind, dflt, when, what) unsetenv(name); rows++;
  FA_KNOBS(FA_UNSET)
#undef FA_UNSET
  const bool only_defaults = argc > 1 && std::string(argv[1]) == "defaults";
  if (only_defaults) defaults(); else values_and_disciplines();
  if (only_defaults && checks != rows) { failures++; fprintf(stderr, "FAILED: %d rows in the table, %d defaults checked\n", rows, checks); }
  printf("%d knobs, %d checks (%s)\n", rows, checks, only_defaults ? "defaults" : "values and read times");
  if (failures) { printf("%d checks FAILED\n", failures); return 1; }
  printf("all checks passed\n");
  return 0;
}
