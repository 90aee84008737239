// fa_diag.h -- the two debug read-outs of a query pass, in ONE table each: the 24 slots of fa_mapper_last_timings and the 29
// fields of fa_mapper_debug_spec.  Plain C++ (no HIP, standard headers only).  The engine generates its enum and its array
// from the tables, pyfastani_amd/diagnostics.py holds the same names for every Python reader, and
// tests/test_diagnostics_host.py holds the two against each other.  include/fastani_hip.h describes what each entry means;
// bench.py reads the timing slots by index, which is why their layout is pinned below.

#pragma once

// A row is X(ENUMERATOR, python_name), in slot order: Workspace::last_ms[ENUMERATOR] is slot `python_name` of
// fa_mapper_last_timings.  MS_STAGE + 0..3 are the four stage times, MS_HOST + 0..2 the host-side split of fa_mapper_query;
// MS_L1_SORTED / MS_L1_MERGED are FA_L1_STATS samples, MS_L1_OFF_FAST counts the fragments that left k_l1's fast form.
// Nothing writes the two unused slots.
#define FA_TIMING_SLOTS(X)       \
  X(MS_SKETCH, sketch_ms)        \
  X(MS_L1, l1_ms)                \
  X(MS_L2, l2_ms)                \
  X(MS_CGI, cgi_ms)              \
  X(MS_TOTAL, total_ms)          \
  X(MS_RECORDS, records)         \
  X(MS_LOCI, loci)               \
  X(MS_EVENTS, events)           \
  X(MS_WIDE, wide_loci)          \
  X(MS_REPEATS, repeats)         \
  X(MS_PACK, pack_ms)            \
  X(MS_TABLES, tables_ms)        \
  X(MS_UPLOAD, upload_ms)        \
  X(MS_CALL, call_ms)            \
  X(MS_UNUSED_14, unused_14)     \
  X(MS_UNUSED_15, unused_15)     \
  X(MS_L2_EVENTS, l2_event_ms)   \
  X(MS_FUSED, fused)             \
  X(MS_UNFUSED, unfused)         \
  X(MS_ORDERED, ordered)         \
  X(MS_L1_SORTED, l1_sorted)     \
  X(MS_L1_MERGED, l1_merged)     \
  X(MS_L1_OFF_FAST, left_fast)   \
  X(MS_TILE_LEN, tile_len)

#define FA_TIMING_ENUMERATOR(id, name) id,
enum TimingSlot : int { FA_TIMING_SLOTS(FA_TIMING_ENUMERATOR) MS_SLOTS, MS_STAGE = MS_SKETCH, MS_HOST = MS_PACK };
#undef FA_TIMING_ENUMERATOR
static_assert(MS_STAGE == 0 && MS_TOTAL == 4 && MS_HOST == 10 && MS_CALL == 13 && MS_L2_EVENTS == 16, "the layout of fa_mapper_last_timings is ABI");
static_assert(MS_REPEATS == 9 && MS_ORDERED == 19 && MS_TILE_LEN == 23 && MS_SLOTS == 24, "the layout of fa_mapper_last_timings is ABI");

// A row is X(python_name, expression), in the order of fa_mapper_debug_spec's out[]: the expression is over the mapper's
// speculation record `s` (fa::Spec), the kernel forms `f` of the last accepted part (fa::Forms) and ppm(share), parts per
// million of a share of fragments.  fa_mapper_debug_spec is the one expansion.
#define FA_SPEC_FIELDS(X)                     \
  X(init, s.init)                             \
  X(smax, s.smax)                             \
  X(seed_slots, s.seed_slots)                 \
  X(small_ppm, ppm(s.l1_small_share))         \
  X(mid_ppm, ppm(s.l1_mid_share))             \
  X(tiny_ppm, ppm(s.l1_tiny_share))           \
  X(l1_prefilter, s.l1_prefilter)             \
  X(l1_no_small, s.l1_no_small)               \
  X(l2_loci_last, s.l2_loci_last)             \
  X(redo, s.redo)                             \
  X(part_frags, s.part_frags)                 \
  X(fuse_skip, s.fuse_skip)                   \
  X(fuse_penalty, s.fuse_penalty)             \
  X(smax_misses, s.smax_misses)               \
  X(scratch_words, (int64_t)s.scratch_words)  \
  X(items_cap, (int64_t)s.items_cap)          \
  X(l_cap, s.l_cap)                           \
  X(n_l1, f.n_l1)                             \
  X(l1_t0, f.l1_threads[0])                   \
  X(l1_t1, f.l1_threads[1])                   \
  X(l1_t2, f.l1_threads[2])                   \
  X(f_prefilter, f.prefilter)                 \
  X(f_scan_sorted, f.scan_sorted)             \
  X(f_wide, f.wide)                           \
  X(f_fused, f.fused)                         \
  X(f_ordered, f.ordered)                     \
  X(f_redo, f.redo)                           \
  X(f_smax, f.smax)                           \
  X(f_seed_slots, f.seed_slots)

#define FA_SPEC_COUNT(name, expr) +1
static_assert(0 FA_SPEC_FIELDS(FA_SPEC_COUNT) == 29, "fa_mapper_debug_spec documents 29 entries (include/fastani_hip.h)");
#undef FA_SPEC_COUNT
