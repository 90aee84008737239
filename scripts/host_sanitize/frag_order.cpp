// frag_order.cpp -- the one-genome workgroup order of k_l2_events (csrc/fa_policy.h: one_genome_run, one_genome_frag) on the
// CPU, under AddressSanitizer + UBSan (tests/test_frag_order_host.py builds and runs it).  A pass inside one genome takes the
// order as arithmetic on the workgroup number, so nothing on the device checks it against a table; this does, for every F from
// the gate (64) to 4096:
//   - the closed form visits every fragment 0 .. F-1 exactly once over the 8 x run workgroups of the grid;
//   - every other workgroup of the grid, and every workgroup behind it, gets -1;
//   - it is the placement the order was defined by (fragment i at (i % run) * 8 + i / run), written out here a second time;
//   - it equals the table of build_frag_order entry by entry -- for a pass that is a whole batch of one genome, and for one
//     that is the second genome of a batch (non-zero first fragment: the table holds numbers relative to the pass).
// Under the gate there is no order: run 0, and build_frag_order returns 0.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../pyfastani_amd/csrc/fa_policy.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; if (failures <= 20) { fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

int main() {
  using namespace fa;
  long checked = 0;
  std::vector<int32_t> table, by_definition;
  std::vector<uint8_t> seen;
  CHECK(one_genome_run(0) == 0 && one_genome_frag(0, 0) == -1, "an empty pass");
  for (int64_t F = 1; F < 64; F++) {
    CHECK(one_genome_run(F) == 0, "F=%lld: a run under the gate", (long long)F);
    const int64_t lo[2] = {0, F};
    CHECK(build_frag_order(lo, 0, 0, F, table) == 0 && table.empty(), "F=%lld: a table under the gate", (long long)F);
  }
  for (int64_t F = 64; F <= 4096; F++) {
    const uint32_t run = one_genome_run(F), grid = 8 * run;
    CHECK(run == (uint32_t)((F + 7) / 8) && grid >= F && grid < F + 8, "F=%lld: run %u", (long long)F, run);
    seen.assign((size_t)F, 0);
    int64_t empty = 0;
    for (uint32_t b = 0; b < grid; b++) {
      const int32_t f = one_genome_frag(b, run, (uint32_t)F);
      CHECK(f == one_genome_frag(b, (uint32_t)F), "F=%lld b=%u: the two forms differ", (long long)F, b);
      if (f < 0) { CHECK(f == -1, "F=%lld b=%u: %d", (long long)F, b, f); empty++; continue; }
      CHECK(f < F, "F=%lld b=%u: fragment %d", (long long)F, b, f);
      if (f < F) { CHECK(!seen[(size_t)f], "F=%lld: fragment %d twice", (long long)F, f); seen[(size_t)f] = 1; }
      // the XCD of a fragment (b mod 8) is its run, and it is the (b / 8)-th of the run
      CHECK((uint32_t)f / run == (b & 7u) && (uint32_t)f % run == b / 8, "F=%lld b=%u: fragment %d off its run", (long long)F, b, f);
    }
    CHECK(empty == (int64_t)grid - F, "F=%lld: %lld empty workgroups of %u", (long long)F, (long long)empty, grid);
    for (int64_t f = 0; f < F; f++) CHECK(seen[(size_t)f], "F=%lld: fragment %lld not visited", (long long)F, (long long)f);
    for (uint32_t b = grid; b < grid + 16; b++) CHECK(one_genome_frag(b, run, (uint32_t)F) == -1, "F=%lld b=%u behind the grid", (long long)F, b);
    // the definition, a second time
    by_definition.assign((size_t)grid, -1);
    for (int64_t i = 0; i < F; i++) by_definition[(size_t)((i % run) * 8 + i / run)] = (int32_t)i;
    // the table: the pass is the whole batch | the second of two genomes
    const int64_t whole[2] = {0, F}, second[3] = {0, 37, 37 + F};
    for (int form = 0; form < 2; form++) {
      const uint32_t n = form == 0 ? build_frag_order(whole, 0, 0, F, table) : build_frag_order(second, 1, 37, 37 + F, table);
      CHECK(n == grid && table.size() == (size_t)grid, "F=%lld form %d: a table of %u for a grid of %u", (long long)F, form, n, grid);
      if (table.size() != (size_t)grid) continue;
      for (uint32_t b = 0; b < grid; b++) {
        CHECK(table[b] == one_genome_frag(b, run, (uint32_t)F), "F=%lld form %d b=%u: table %d", (long long)F, form, b, table[b]);
        CHECK(table[b] == by_definition[b], "F=%lld form %d b=%u: table %d, defined as %d", (long long)F, form, b, table[b], by_definition[b]);
        checked++;
      }
    }
    CHECK(frag_range_in_one_genome(whole, 0, 0, F) && frag_range_in_one_genome(second, 1, 37, 37 + F) && frag_range_in_one_genome(second, 0, 37, 37 + F) &&
          !frag_range_in_one_genome(second, 0, 36, 37 + F) && !frag_range_in_one_genome(second, 0, 0, 38), "F=%lld: one genome or several", (long long)F);
  }
  if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
  printf("all checks passed (%ld table entries)\n", checked);
  return 0;
}
