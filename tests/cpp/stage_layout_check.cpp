// stage_layout_check.cpp — the block layout of the host forms' staging (mtgpu::stage_layout, csrc/api_common.h) on random
// combinations of present and absent inputs and outputs: every slot 256-byte aligned, no two slots overlapping, no slot
// for what is absent, the slots summing to the reserved size — and the offsets and the size equal to the formulas that
// mtgpu_scan_frames_blobs, mtgpu_scan_frames_dir, mtgpu_activity_map and the plain scan wrote out by hand before the
// helper existed (copied below from those functions).  Built with -fsanitize=address,undefined by
// tests/test_stage_layout_host.py; no HIP, no library.
//
// Usage: stage_layout_check [rounds [seed]]   prints "ok <layouts> layouts" or the first mismatch; exit 0 / 1.
#define MTGPU_STAGE_LAYOUT_ONLY
#include "api_common.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using mtgpu::kNoSlot;
using mtgpu::StageSlot;

namespace {

int n_slots = 0;
StageSlot slot[mtgpu::kStageMaxSlots];
size_t off[mtgpu::kStageMaxSlots];

// Staged::in / Staged::out of csrc/api_common.h, restated: an input that is not given has 0 bytes; an output that is not
// asked for has no slot unless `always`.
int in(bool given, size_t bytes) { slot[n_slots] = {given ? bytes : 0u, true}; return n_slots++; }
int out(bool asked, size_t bytes, bool always = false) { slot[n_slots] = {bytes, asked || always}; return n_slots++; }

size_t up(size_t v) { return (v + 255u) & ~(size_t)255u; }

int fail(const char *what, unsigned long long round) {
  std::printf("MISMATCH in round %llu: %s\n", round, what);
  return 1;
}

// what holds for every layout
const char *check_generic(size_t total, bool exact_tail) {
  size_t sum = 0, last_end = 0;
  for (int i = 0; i < n_slots; ++i) {
    if (!slot[i].present) { if (off[i] != kNoSlot) return "an absent slot has an offset"; continue; }
    if (off[i] == kNoSlot) return "a present slot has no offset";
    if (off[i] % 256u != 0) return "a slot is not 256-byte aligned";
    if (off[i] != sum) return "a slot does not begin where the one before it ends";
    for (int j = 0; j < i; ++j)
      if (slot[j].present && slot[j].bytes && slot[i].bytes && off[j] + slot[j].bytes > off[i]) return "two slots overlap";
    last_end = off[i] + slot[i].bytes;
    sum += up(slot[i].bytes);
  }
  if (total != (exact_tail ? last_end : sum)) return "the slots do not sum to the reserved size";
  return nullptr;
}

}  // namespace

int main(int argc, char **argv) {
  const unsigned long long rounds = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 4000ull;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 23ull);
  unsigned long long layouts = 0;
  for (unsigned long long r = 0; r < rounds; ++r) {
    // sizes around the 256-byte steps, small and large
    const size_t n_frames = 1 + (size_t)(rng() % (r % 3 == 0 ? 70000u : 600u));
    const size_t n_streams = 1 + (size_t)(rng() % 40u), gh = 1 + (size_t)(rng() % 140u), gw = 1 + (size_t)(rng() % 260u);
    const size_t W = (gw + 63u) / 64u;
    const bool keep = rng() & 1, flags = rng() & 1, centres = rng() & 1, blobs = rng() & 1, largest = rng() & 1, box = rng() & 1,
               rose = rng() & 1;
    const size_t words = 4u * n_frames;
    const char *bad;

    {  // mtgpu_scan_frames_blobs (d_misc): stream_off | keep | flags | centres | blobs | largest | box
      const size_t keep_bytes = keep ? 8u * n_streams * gh * W : 0;
      const size_t soff_bytes = keep ? 8u * (n_streams + 1) : 0;
      const size_t o_soff = 0, o_keep = o_soff + up(soff_bytes), o_fl = o_keep + up(keep_bytes), o_cen = o_fl + (flags ? up(n_frames) : 0),
                   o_bl = o_cen + (centres ? up(words) : 0), o_lg = o_bl + (blobs ? up(words) : 0), o_box = o_lg + (largest ? up(words) : 0),
                   total = o_box + (box ? up(8u * n_frames) : 0);
      n_slots = 0;
      // without a mask the caller passes null pointers and n_streams 0
      const int i_soff = in(keep, 8u * ((keep ? n_streams : 0) + 1)), i_keep = in(keep, 8u * (keep ? n_streams : 0) * gh * W);
      const int a = out(flags, n_frames), b = out(centres, words), c = out(blobs, words), d = out(largest, words), e = out(box, 8u * n_frames);
      const size_t got = mtgpu::stage_layout(slot, n_slots, false, off);
      if ((bad = check_generic(got, false))) return fail(bad, r);
      if (got != total || off[i_soff] != o_soff || off[i_keep] != o_keep || (flags && off[a] != o_fl) || (centres && off[b] != o_cen) ||
          (blobs && off[c] != o_bl) || (largest && off[d] != o_lg) || (box && off[e] != o_box))
        return fail("not the layout of mtgpu_scan_frames_blobs", r);
      ++layouts;
    }
    {  // mtgpu_scan_frames_dir (d_misc): stream_off | allows | flags | centres | rose
      const bool allows = keep;
      const size_t soff_bytes = allows ? 8u * (n_streams + 1) : 0, allow_bytes = allows ? n_streams : 0;
      const size_t rose_bytes = 32u * n_frames;
      const size_t o_soff = 0, o_allow = o_soff + up(soff_bytes), o_fl = o_allow + up(allow_bytes), o_cen = o_fl + (flags ? up(n_frames) : 0),
                   o_rose = o_cen + (centres ? up(words) : 0), total = o_rose + (rose ? up(rose_bytes) : 0);
      n_slots = 0;
      const int i_soff = in(allows, 8u * ((allows ? n_streams : 0) + 1)), i_allow = in(allows, allows ? n_streams : 0);
      const int a = out(flags, n_frames), b = out(centres, words), c = out(rose, rose_bytes);
      const size_t got = mtgpu::stage_layout(slot, n_slots, false, off);
      if ((bad = check_generic(got, false))) return fail(bad, r);
      if (got != total || off[i_soff] != o_soff || off[i_allow] != o_allow || (flags && off[a] != o_fl) || (centres && off[b] != o_cen) ||
          (rose && off[c] != o_rose))
        return fail("not the layout of mtgpu_scan_frames_dir", r);
      ++layouts;
    }
    {  // mtgpu_activity_map (d_misc): stream_off | active | centre | frames — the room of `frames` stands with or without it
      const size_t plane = 4u * n_streams * gh * gw;
      const bool active = flags, centre = centres, frames = blobs;
      const size_t o_soff = 0, o_act = o_soff + up(8u * (n_streams + 1)), o_cen = o_act + (active ? up(plane) : 0),
                   o_fr = o_cen + (centre ? up(plane) : 0), total = o_fr + up(4u * n_streams);
      n_slots = 0;
      const int i_soff = in(true, 8u * (n_streams + 1));
      const int a = out(active, plane), b = out(centre, plane), c = out(frames, 4u * n_streams, true);
      const size_t got = mtgpu::stage_layout(slot, n_slots, false, off);
      if ((bad = check_generic(got, false))) return fail(bad, r);
      if (got != total || off[i_soff] != o_soff || (active && off[a] != o_act) || (centre && off[b] != o_cen) || off[c] != o_fr)
        return fail("not the layout of mtgpu_activity_map", r);
      ++layouts;
    }
    {  // mtgpu_scan_frames / _centres (d_flags, sized to the last byte): [flags n_frames | pad to 256 | centres n_frames x 4]
      const size_t centres_at = (n_frames + 255u) & ~(size_t)255u;
      const size_t total = centres ? centres_at + 4u * n_frames : n_frames;
      n_slots = 0;
      const int a = out(flags, n_frames, true), b = out(centres, words);
      const size_t got = mtgpu::stage_layout(slot, n_slots, true, off);
      if ((bad = check_generic(got, true))) return fail(bad, r);
      if (got != total || off[a] != 0 || (centres && off[b] != centres_at)) return fail("not the layout of the plain scan's d_flags", r);
      ++layouts;
    }
  }
  std::printf("ok %llu layouts\n", layouts);
  return 0;
}
