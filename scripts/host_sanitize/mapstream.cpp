// The window arithmetic of the streamed mapping output (pyfastani_amd/csrc/fa_mapstream.h) against a brute-force model, on the
// CPU: build with  g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all mapstream.cpp  and run.
//
// For every total 0..300 and every stage 1..130: the windows partition [0, total) in order and none is empty.  For chunkings of
// the records drawn at random (empty chunks included): map_chunk_in_window keeps exactly the chunks that hold a record of the
// window, and a model of k_map_write -- every kept chunk writes its records of the window to place - lo -- fills every slot of
// every window exactly once, with the right record, and nothing beyond the stage.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pyfastani_amd/csrc/fa_mapstream.h"

static int failures = 0;
#define CHECK(cond, ...) \
  do { if (!(cond)) { if (failures++ < 20) { fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int main() {
  long windows_checked = 0, chunks_checked = 0;
  for (int64_t total = 0; total <= 300; total++) {
    // three chunkings per total: counts of a chunk 0..7, 0..70, and all records in one chunk between empty ones
    std::vector<std::vector<int64_t>> chunkings;
    for (int kind = 0; kind < 3; kind++) {
      std::vector<int64_t> counts;
      int64_t left = total;
      if (kind == 2) { counts = {0, total, 0}; left = 0; }
      while (left > 0) {
        int64_t c = (int64_t)(rnd() % (kind == 0 ? 8 : 71));
        if (c > left) c = left;
        counts.push_back(c);
        left -= c;
      }
      counts.push_back(0);
      chunkings.push_back(counts);
    }
    for (int64_t stage = 1; stage <= 130; stage++) {
      const int64_t n_win = fa::map_windows(total, stage);
      CHECK((total == 0) == (n_win == 0), "total %lld stage %lld: %lld windows", (long long)total, (long long)stage, (long long)n_win);
      int64_t next = 0;
      for (int64_t w = 0; w < n_win; w++) {
        const fa::MapWindow win = fa::map_window(total, stage, w);
        CHECK(win.lo == next && win.hi > win.lo && win.hi - win.lo <= stage && win.hi <= total,
              "total %lld stage %lld window %lld = [%lld, %lld)", (long long)total, (long long)stage, (long long)w, (long long)win.lo, (long long)win.hi);
        CHECK(w + 1 == n_win || win.hi - win.lo == stage, "a window in front of the last is not full");
        next = win.hi;
        windows_checked++;
        for (const std::vector<int64_t> &counts : chunkings) {
          std::vector<int64_t> slot((size_t)stage, -1);     // the stage buffer: which record lies in every slot
          int64_t off = 0;
          for (size_t b = 0; b < counts.size(); b++) {
            bool holds = false;                              // brute force: some place of the chunk lies in the window
            for (int64_t o = off; o < off + counts[b]; o++) holds = holds || (o >= win.lo && o < win.hi);
            const bool kept = fa::map_chunk_in_window(off, counts[b], win.lo, win.hi);
            CHECK(kept == holds, "chunk [%lld, +%lld) window [%lld, %lld): kept %d holds %d", (long long)off, (long long)counts[b],
                  (long long)win.lo, (long long)win.hi, (int)kept, (int)holds);
            if (kept)
              for (int64_t o = off; o < off + counts[b]; o++) {
                if (o < win.lo || o >= win.hi) continue;
                CHECK(o - win.lo >= 0 && o - win.lo < stage && slot[(size_t)(o - win.lo)] == -1, "place %lld written twice or out of the stage", (long long)o);
                slot[(size_t)(o - win.lo)] = o;              // (under ASan an index beyond the stage is a finding of its own)
              }
            off += counts[b];
            chunks_checked++;
          }
          CHECK(off == total, "the chunking holds %lld of %lld records", (long long)off, (long long)total);
          for (int64_t i = 0; i < stage; i++)
            CHECK(slot[(size_t)i] == (i < win.hi - win.lo ? win.lo + i : -1), "slot %lld of window %lld holds %lld", (long long)i, (long long)w, (long long)slot[(size_t)i]);
        }
      }
      CHECK(next == total, "the windows end at %lld of %lld", (long long)next, (long long)total);
    }
  }
  // sizes beyond 32 bits: the arithmetic is 64-bit throughout
  {
    const int64_t total = (1LL << 40) + 5, stage = (1LL << 31) + 3;
    const int64_t n_win = fa::map_windows(total, stage);
    const fa::MapWindow last = fa::map_window(total, stage, n_win - 1);
    CHECK(last.hi == total && last.lo == (n_win - 1) * stage && last.hi - last.lo >= 1 && last.hi - last.lo <= stage, "large sizes");
    CHECK(fa::map_windows(INT64_MAX, 1) == INT64_MAX && fa::map_windows(INT64_MAX, INT64_MAX) == 1, "largest sizes");
  }
  printf("%ld windows, %ld chunk decisions\n", windows_checked, chunks_checked);
  if (failures) { printf("%d checks FAILED\n", failures); return 1; }
  printf("all checks passed\n");
  return 0;
}
