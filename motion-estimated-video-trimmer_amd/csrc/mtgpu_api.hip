// mtgpu_api.hip — implementation of the C ABI declared in include/mtgpu.h:
// parameter derivation, launch planning, host<->device staging.  The compute is
// in scan_kernels.hip / merge_kernels.hip; nothing here computes a result on
// the CPU (no fallback: without a usable device every compute call fails).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cctype>
#include <condition_variable>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

#include "../../include/mtgpu.h"
#include "api_internal.h"
#include "knobs.h"
#include "pack_simd.h"
#include "merge_kernels.h"
#include "scalar_kernels.h"
#include "scan_kernels.h"
#include "sweep_kernels.h"
#include "activity_kernels.h"
#include "zones_kernels.h"
#include "blobs_kernels.h"
#include "gmc_kernels.h"
#include "gmc_blobs_kernels.h"
#include "persist_kernels.h"
#include "tracks_kernels.h"
#include "dir_kernels.h"
#include "lanes_kernels.h"
#include "objects_kernels.h"
#include "headings_kernels.h"

namespace {
thread_local char g_err[512] = "";
}

namespace mtgpu {

int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

int hip_fail(hipError_t e, const char *what) {
  return fail(MT_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
}

}  // namespace mtgpu

namespace {

using mtgpu::fail;
using mtgpu::hip_fail;

#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t _e = (expr);                             \
    if (_e != hipSuccess) return hip_fail(_e, #expr);   \
  } while (0)

// Grow-only device buffer used by the host-pointer entry points.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  int reserve(size_t bytes) {
    if (bytes <= cap) return MT_OK;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) { p = nullptr; return hip_fail(e, "hipMalloc(staging)"); }
    cap = want;
    return MT_OK;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

}  // namespace

struct mtgpu_ctx {
  mt_scan_params params;
  mtgpu::ScanK k;
  mtgpu_plan plan;
  int device;            // physical HIP device
  int logical_device = 0;  // what the caller asked for (differs only under MTGPU_ALIAS_DEVICES)
  hipStream_t stream;    // private stream of the host-pointer entry points
  std::atomic<int> slices_request{0};  // 0 = auto, else 1/2/4/8 (mtgpu_set_slices, MTGPU_FORCE_SLICES): read once per launch,
                                       // may be set while other threads scan through this context
  int wide_chunk_rows = 0, wide_lds_bytes = 0;   // single-workgroup-per-CU layout (see make_plan)
  int item_chunk = 0;    // MTGPU_ITEM_CHUNK (tests): workgroups per kernel launch, 0 = 2^30
  int lds_max = 0;       // device limit of LDS per workgroup
  int group_request = 0; // MTGPU_GROUP: frames per workgroup, 0 = automatic
  int per_cu_request = 0; // MTGPU_WG_PER_CU: 1 | 2 = at most that many scan workgroups per CU on every launch, -1 = never
                          // fewer than the tile allows, 0 = automatic (choose_lds_floor)
  int early_exit = 0;    // the plan allows the scan's early exit (make_plan; MTGPU_EARLY_EXIT=0 switches it off): launch_scan_on
                         // then sets ScanK::early on every launch that qualifies — 1: with eight frames per CU or more, 2: any size
  int check_offsets = 0; // MTGPU_CHECK_OFFSETS=1: the device entry points verify "frame_off non-decreasing" first (one sync per call)
  // Launch scratch (work lists of the device entry points, spill queues, slice tiles, merge workspaces): a ring of
  // device blocks, each with the event of its last user.  Whoever takes a block makes ITS stream wait for that event,
  // so a block never has two users at once, whatever streams and threads the launches come from.  (Through round 5
  // this was a hipMemPool with hipMallocFromPoolAsync / hipFreeAsync.  Round 6 made every launch use scratch, and 16
  // host threads on their own streams then saw launches trample each other's work lists — one wrong flag in a few
  // hundred launches, also with a mutex around the pool calls, also with one stream per batch; with memory that a
  // launch demonstrably owns, none: profiles/r06_host_stress_*.log.  The library no longer relies on cross-stream
  // reuse inside the runtime's stream-ordered allocator.)
  struct Scratch {
    static constexpr int kSlots = 16;
    static constexpr size_t kBig = 64u << 20;   // requests from here on wait for a block that is large enough rather than grow another
    struct Slot {
      void *p = nullptr; size_t cap = 0;
      hipEvent_t ev = nullptr;          // recorded behind the last launch that used the block
      hipStream_t last = nullptr;       // ... and the stream it ran on (a preference only: the event is waited for regardless)
      bool recorded = false;
      bool busy = false;                // a host thread is queueing work that uses the block (guarded by mu; the other
    };                                  // fields of a busy slot belong to that thread)
    std::mutex mu;
    std::condition_variable cv;
    Slot slot[kSlots];
    uint64_t reserved = 0, reserved_high = 0;
  } scratch;
  uint64_t merge_large_min = 4096;   // timestamp lists at least this long take the multi-workgroup merge (MTGPU_MERGE_LARGE_MIN)
  // Streams of the pipes (host dispatcher): ONE small pool per context, handed to staging batches round-robin,
  // instead of a stream per batch.  Creating a HIP stream costs ~3.5 ms and the runtime serialises it: 64 workers
  // x 3 batches = 192 streams took 0.68 s of wall time and 0.35 s per worker — THE cost of creating a pipe
  // (profiles/r04_pin_probe2.json) — while the runtime maps streams onto a handful of hardware queues anyway.
  static constexpr int kMaxPipeStreams = 8;
  hipStream_t pipe_streams[kMaxPipeStreams] = {};
  unsigned pipe_rr = 0;                  // next slot (guarded by pipe_mu)
  std::mutex pipe_mu;
  std::mutex mu;         // guards the staging buffers below
  DevBuf d_mv, d_off, d_sd, d_flags, d_misc;
  // launch timing (mtgpu_profile_enable): a ring of event triples {before planning, planned, scanned}
  struct Profile {
    static constexpr int kRing = 64;
    std::atomic<int> on{0};
    std::mutex mu;                       // held across a profiled launch
    hipEvent_t ev[kRing][3] = {};
    bool created = false;
    int tail = 0, count = 0;             // outstanding triples: tail .. tail + count - 1 (mod kRing)
    double plan_ms = 0.0, scan_ms = 0.0;
    uint32_t launches = 0;
    // waits for the oldest outstanding triple and adds its times up (mu held)
    hipError_t drain_one() {
      hipEvent_t *t = ev[tail];
      hipError_t e = hipEventSynchronize(t[2]);
      if (e != hipSuccess) return e;
      float a = 0.f, b = 0.f;
      if ((e = hipEventElapsedTime(&a, t[0], t[1])) != hipSuccess) return e;
      if ((e = hipEventElapsedTime(&b, t[1], t[2])) != hipSuccess) return e;
      plan_ms += a; scan_ms += b; ++launches;
      tail = (tail + 1) % kRing; --count;
      return hipSuccess;
    }
  } prof;
};

namespace {

// keep an MV iff !(mag_sq < T) with mag_sq a non-negative integer (src/motion_scanner.cpp:251)
//   <=>  mag_sq >= ceil(T)   (T NaN or <= 0: keep all;  T above any reachable mag_sq: keep none)
unsigned long long threshold_to_int(double t) {
  if (!(t > 0.0)) return 0ull;                       // NaN, 0, negative
  if (t > 17179869184.0) return ~0ull;               // > 2^34 > 2 * 65535^2: unreachable
  return (unsigned long long)std::ceil(t);
}

// The synchronous entry points queue copies from / to CALLER memory: whatever way they return, the
// stream has drained first, so the caller may free its buffers right away (also after an error).
struct DrainOnExit {
  hipStream_t st;
  ~DrainOnExit() { (void)hipStreamSynchronize(st); }
};

int validate_params(const mt_scan_params *p) {
  if (!p) return fail(MT_ERR_INVALID, "params is NULL");
  if (p->grid_w < 1 || p->grid_h < 1 || p->grid_w > 32767 || p->grid_h > 32767)
    return fail(MT_ERR_INVALID, "grid %dx%d outside [1,32767] (int16 in the reference)", p->grid_w, p->grid_h);
  if (p->block_shift < 0 || p->block_shift > 31)
    return fail(MT_ERR_INVALID, "block_shift %d outside [0,31]", p->block_shift);
  if (p->vertical_margin < 0)
    return fail(MT_ERR_INVALID, "vertical_margin %d < 0 (the reference would index before the grid)", p->vertical_margin);
  return MT_OK;
}

// LDS bytes of one workgroup: packed counters for (band_rows + 2) rows, a mask buffer for
// (chunk_rows + 2) rows, the centre total.
size_t lds_need(int band_rows, int chunk_rows, int gw, int W, int fb, int *cnt_words) {
  const size_t fields = (size_t)(band_rows + 2) * (size_t)gw;
  size_t cw = (fields * (size_t)fb + 31u) / 32u;
  cw = (cw + 3u) & ~(size_t)3u;
  if (cnt_words) *cnt_words = (int)cw;
  return cw * 4u + (size_t)(chunk_rows + 2) * (size_t)W * 8u + 16u;
}

using mtgpu::env_int;

int make_plan(mtgpu_ctx *c, int lds_max, int cu_count) {
  const mt_scan_params &p = c->params;
  mtgpu::ScanK &k = c->k;
  k.thr = threshold_to_int(p.mv_threshold_sq);
  k.shift = p.block_shift;
  k.gw = p.grid_w;
  k.gh = p.grid_h;
  k.y_lo = p.vertical_margin;                                // :237
  k.y_hi = p.grid_h - p.vertical_margin;                     // :238
  if (k.y_hi < k.y_lo) k.y_hi = k.y_lo;                      // empty analysed range
  k.vec_need = p.vectors_needed;
  k.clust_need = p.clusters_needed < 1 ? 1u : (unsigned int)p.clusters_needed;
  k.W = (p.grid_w + 63) / 64;
  const int R = (k.y_hi - k.y_lo) < 1 ? 1 : (k.y_hi - k.y_lo);
  const size_t mask_row = (size_t)k.W * 8u;

  // Counter form (scan_kernels.hip).  Plain 32-bit adds whenever the whole tile fits LDS (the
  // fastest and contention-proof form); otherwise packed thermometer fields, the narrowest of
  // 1/2/4/8 bits >= vectors_needed; binary 8-bit CAS fields only for vectors_needed > 8.
  // MTGPU_FORCE_FB = 32 | 1 | 2 | 4 | 8 | 108 (8-bit CAS) overrides, for tests and experiments.
  const unsigned int vn = k.vec_need;
  int packed_fb = vn <= 1u ? 1 : (vn <= 2u ? 2 : (vn <= 4u ? 4 : 8));
  int packed_mode = vn <= 8u ? 1 : 2;
  int fb = 32, mode = 0;
  if (lds_need(R, R, k.gw, k.W, 32, nullptr) > (size_t)lds_max) { fb = packed_fb; mode = packed_mode; }
  const int force = env_int("MTGPU_FORCE_FB", 0);
  if (force == 32) { fb = 32; mode = 0; }
  else if (force == 108) { fb = 8; mode = 2; }
  else if ((force == 1 || force == 2 || force == 4 || force == 8) && (unsigned int)force >= vn) { fb = force; mode = 1; }
  else if (force == 1 || force == 2 || force == 4 || force == 8) { fb = packed_fb; mode = packed_mode; }
  k.mode = mode;
  k.active_min = mode == 1 ? ((1u << vn) - 1u) : vn;         // thermometer full / binary count

  int band_rows = R, chunk_rows = R;
  if (lds_need(R, R, k.gw, k.W, fb, nullptr) > (size_t)lds_max) {
    // 1st choice: whole grid in one tile, phase 2 in row chunks through a smaller mask buffer
    const size_t cnt_only = lds_need(R, -2, k.gw, k.W, fb, nullptr);   // counters + total
    const long room = (long)lds_max - (long)cnt_only;
    long ch = room / (long)mask_row - 2;
    if (ch > R) ch = R;
    if (ch >= 8 || ch >= R) {
      chunk_rows = (int)ch;
    } else {
      // 2nd choice: row bands walked by ONE workgroup per frame (scan_kernels.hip, SPILL): the
      // records are still read once; later bands replay the queued votes.  As few, as large
      // bands as LDS allows: one workgroup per CU then owns the CU's whole bandwidth, so a frame
      // is finished (and the next one started) in half the time two co-resident workgroups would
      // need — with 20 MB work units that halves the idle tail of a launch (960x540, 1024 frames:
      // 2 bands 6.8 TB/s vs 4 bands 6.3-6.6), and every band less is one queue replay less on
      // vote-heavy input (pan: 5.1 vs 4.1 TB/s).
      const size_t per_row = ((size_t)k.gw * (size_t)fb + 7u) / 8u + mask_row;
      long r = ((long)lds_max - 64) / (long)per_row - 2;
      while (r >= 1 && lds_need((int)r, (int)r, k.gw, k.W, fb, nullptr) > (size_t)lds_max) --r;
      if (r < 1)
        return fail(MT_ERR_CAPACITY, "grid width %d: three counter rows do not fit %d bytes of LDS", k.gw, lds_max);
      if (r > R) r = R;
      const long nb = ((long)R + r - 1) / r;                      // balance the bands
      band_rows = chunk_rows = (int)(((long)R + nb - 1) / nb);
    }
  }
  // Two workgroups per CU hide each other's zero / cluster-test phases (measured +4 % on the
  // 960x540 grid): when only the mask buffer pushes a tile over half of LDS, chunk the cluster
  // test so that the tile fits 80 KB.
  // That only helps when a launch has more work items than CUs; with fewer, one workgroup per
  // CU runs anyway and the single-chunk layout is faster (5.87 vs 5.50 TB/s at 256 frames), so
  // both layouts are kept and launch_scan_on picks per launch.
  c->wide_chunk_rows = chunk_rows;
  c->wide_lds_bytes = (int)lds_need(band_rows, chunk_rows, k.gw, k.W, fb, nullptr);
  {
    const size_t half = 80u * 1024u;
    const size_t cnt_only = lds_need(band_rows, -2, k.gw, k.W, fb, nullptr);
    if (lds_need(band_rows, chunk_rows, k.gw, k.W, fb, nullptr) > half && cnt_only + 10u * mask_row <= half) {
      const long ch = (long)((half - cnt_only) / mask_row) - 2;
      if (ch >= 8 && ch < chunk_rows) chunk_rows = (int)ch;
    }
  }
  k.fb = fb;
  k.band_rows = band_rows;
  k.chunk_rows = chunk_rows;
  k.bands = (R + band_rows - 1) / band_rows;
  k.mask_rows = chunk_rows + 2;
  const size_t lds = lds_need(band_rows, chunk_rows, k.gw, k.W, fb, &k.cnt_words);
  // Workgroup size: 512 threads x 4 loads in flight per lane keep a CU's memory queue full at
  // 4 workgroups/CU (measured +2.5 % over 256 on 1080p); tiles above 48 KB run 1-2
  // workgroups/CU and take 16 waves each.
  // "4 workgroups/CU" is what LDS allows, not what runs: four 512-thread workgroups are 8 waves per SIMD, which a CU
  // admits only up to 80 SGPRs and 64 VGPRs per wave — min(8, floor(800 / (ceil(sgpr / 16) * 16 + 16))) — and every
  // scan kernel takes 106 SGPRs (the compact ones 67-85 VGPRs as well): 6 or 5 waves per SIMD, THREE such workgroups
  // per CU.  Every figure quoted here was taken at three; four, tried in round 22, is slower (scan_kernels.hip), and
  // launches of large frames ask for ONE per CU (choose_lds_floor).
  int block = lds <= 48u * 1024u ? 512 : 1024;
  // MTGPU_FORCE_BLOCK (tests): 512 | 1024.  The library instantiates what the planner can choose plus that switch:
  // 512- and 1024-thread workgroups for single tiles, 1024 for banded plans (their tiles always exceed 48 KB).
  const int fblock = env_int("MTGPU_FORCE_BLOCK", 0);
  if (fblock == 512 || fblock == 1024) block = fblock;
  if (k.bands > 1) block = 1024;
  c->plan.block_threads = block;
  c->plan.bands = k.bands;
  c->plan.band_rows = k.band_rows;
  c->plan.lds_bytes = (int)lds;
  c->plan.counter_bits = fb;
  c->plan.device = c->logical_device;
  c->plan.cu_count = cu_count;
  c->plan.chunk_rows = chunk_rows;
  {
    const int fs = env_int("MTGPU_FORCE_SLICES", 0);
    c->slices_request.store((fs == 1 || fs == 2 || fs == 4 || fs == 8) ? fs : 0, std::memory_order_relaxed);
  }
  k.slices = 1;
  k.group = 1;
  k.sys_flags = 0;                                            // per launch: launch_scan_on
  k.sys_centres = 0;
  k.early = 0;                                                // per launch: launch_scan_on
  // The early exit (scan_kernels.hip, vote_and_prove): its proof counts two centres, found by single 32-bit adds on a
  // tile that tracks every analysed row, with cells that are inactive until they are voted for.  MTGPU_EARLY_EXIT=0
  // (tests, A/B runs) switches it off, =2 takes it on launches of any size (launch_scan_on).
  {
    const int want = env_int("MTGPU_EARLY_EXIT", 1);
    const bool can = k.bands == 1 && fb == 32 && mode == 0 && k.vec_need >= 1u && k.clust_need <= 2u;
    c->early_exit = !can || want == 0 ? 0 : (want == 2 ? 2 : 1);
  }
  c->group_request = env_int("MTGPU_GROUP", 0);
  c->per_cu_request = env_int("MTGPU_WG_PER_CU", 0);
  c->check_offsets = env_int("MTGPU_CHECK_OFFSETS", 0) != 0;
  c->item_chunk = env_int("MTGPU_ITEM_CHUNK", 0);
  if (c->item_chunk < 0) c->item_chunk = 0;
  {
    const int lm = env_int("MTGPU_MERGE_LARGE_MIN", 0);
    if (lm > 0) c->merge_large_min = (uint64_t)lm;
  }
  c->plan.counter_mode = mode;
  c->plan.early_exit = c->early_exit;
  return MT_OK;
}

// Slices per frame for this launch.  Measured (scripts/ab_scan.py, AB_SET=slices): the hand-off
// (tile write + agent-scope release/acquire + tile reads) costs several microseconds per
// workgroup, so splitting pays only for batches that leave most CUs idle AND whose frames are
// large: 64 frames of the 960x540 grid +47 % with 4 slices, 64 4K frames +8 % with 2; every
// other shape loses (256 1080p frames: -40 % with 2).  Auto therefore never exceeds one
// workgroup per CU and keeps >= 32768 records (1.3 MB) per slice.
int choose_slices(const mtgpu_ctx *c, uint64_t n_records, uint32_t n_frames) {
  if (c->k.bands != 1) return 1;
  int s = c->slices_request.load(std::memory_order_relaxed);
  if (s == 0) {                                               // auto
    const uint64_t cus = (uint64_t)(c->plan.cu_count > 0 ? c->plan.cu_count : 256);
    const uint64_t avg = n_records / (n_frames ? n_frames : 1);
    s = 1;
    while (s < 8 && (uint64_t)n_frames * (uint64_t)(2 * s) <= cus && avg / (uint64_t)(2 * s) >= 32768ull) s *= 2;
  }
  return (s == 2 || s == 4 || s == 8) ? s : 1;
}

// Frames per workgroup.  Very short workgroups are started more slowly than they finish (the
// dispatcher starts ~19 per microsecond), so few are alive per CU and nothing overlaps their
// zeroing / cluster test: frames below ~128 KB are scanned two or more per workgroup.  Measured
// after the 32-bit kernels dropped to 58-61 VGPRs (which allows four workgroups per CU; their 106 SGPRs admitted
// three, see make_plan, so the figures here and below are three-per-CU figures): 65 KB frames (1080p,
// one compact record per cell) +5 % with 2-4 per workgroup; 252 KB and 326 KB frames are 2-3 %
// FASTER one per workgroup (the earlier 1 MB target dated from two workgroups per CU).
// Only for batches that fill the chip several times over.
int choose_group(const mtgpu_ctx *c, uint64_t n_records, uint32_t n_frames, int rec_bytes, int slices) {
  if (slices != 1 || n_frames == 0) return 1;
  int g = c->group_request;
  if (g <= 0) {
    const uint64_t avg = n_records * (uint64_t)rec_bytes / n_frames;
    const uint64_t cus = (uint64_t)(c->plan.cu_count > 0 ? c->plan.cu_count : 256);
    g = 1;
    // round 3, 40-byte records at 21 GB per launch: 48 KB frames (480p, one record per cell) 5.98 / 6.28 / 6.48 /
    // 6.70 TB/s with 1 / 2 / 4 / 8 frames per workgroup, 144 KB frames (720p) 7.01 / 7.15 / 7.19 / 7.13, 192 KB
    // frames (480p dense8x8) 7.22 / 7.08 / 7.04: frames up to ~160 KB are grouped up to ~600 KB per workgroup
    if (avg <= 160ull * 1024ull)
      while (g < 8 && avg * (uint64_t)(2 * g) <= 600ull * 1024ull && (uint64_t)n_frames >= cus * 8ull * (uint64_t)(2 * g)) g *= 2;
    // Compact records on a tile that leaves ONE workgroup per CU (4K: 124 KB of 32-bit counters): nothing overlaps
    // that workgroup's zeroing and cluster test (5 of 38 us per ~1 MB frame), so it scans 2-4 frames in a row
    // and issues the next frame's first streaming step before its cluster test (scan_kernels.hip, NextStep).
    // Round 3, 4K dense8x8 compact: 1024 frames 6.13 -> 6.39 TB/s, 4096 frames 6.54 -> 6.73; 4 MB frames
    // (960x540) and four-per-CU tiles (1080p) gain nothing or lose, 40-byte records lose 2 % (no prefetch there).
    if (g == 1 && rec_bytes == MT_COMPACT_BYTES && c->plan.lds_bytes > 80 * 1024 && avg <= (2ull << 20)) {
      if ((uint64_t)n_frames >= cus * 4ull) g = 4;
      else if ((uint64_t)n_frames >= cus * 2ull) g = 2;
    }
    // Round 6 (a workgroup that owns several list entries parks them in LDS when it starts and issues the next frame's
    // first loads before this frame's cluster test): profiles/r06_group_ab.log, wall clock per call —
    //   compact records on tiles that share a CU (1080p: 261 KB frames, 37 us per workgroup, of which ~3 us are
    //   start-up): two frames per workgroup 635 -> 594 us at 16 384 frames, 174 -> 160 us at 4096 (four: 601 / 161);
    //   40-byte records on a one-workgroup-per-CU tile (4K: 5.2 MB frames): 2895 -> 2881 us with two on equal frames,
    //   but -3 % on ragged ones (profiles/r06_group_ab.log, second part: 10 MB work units leave a long tail) — not taken;
    //   40-byte records on shared tiles (1080p 1.3 MB frames, 326 KB frames): nothing or a loss — they stay at one.
    // Only where every workgroup slot of the chip is still filled twice over afterwards.
    // (per_cu is what LDS allows.  This rule is about compact records, whose kernels take 106 SGPRs and 67-85 VGPRs:
    //  6 or 5 waves per SIMD, so a <= 40 KB tile really has THREE workgroups per CU, not four, and the bound below is
    //  stricter than "twice over" by a third.  It is left where it was measured.)
    const uint64_t per_cu = c->plan.lds_bytes <= 40 * 1024 ? 4u : (c->plan.lds_bytes <= 80 * 1024 ? 2u : 1u);
    if (g == 1 && c->k.bands == 1 && rec_bytes == MT_COMPACT_BYTES && avg <= (2ull << 20) &&
        (uint64_t)n_frames >= cus * per_cu * 4ull)
      g = 2;
  }
  if (g > 64) g = 64;
  return g < 1 ? 1 : g;
}

// Workgroups per CU for this launch, set through the size of the dynamic LDS: a workgroup that asks for more than
// half of a CU's 160 KB has the CU to itself, more than a third shares it with one other.  Returns the least LDS
// size to ask for (0: whatever the tile needs).
// Round 22, 40-byte records, scan-kernel time at 3 (what the tile and the kernels' 106 SGPRs allow) / 2 / 1 per CU
// (profiles/r22_per_cu_legs.log): streaming LARGE frames, a CU is fastest with ONE workgroup — 256 record streams
// into the memory system instead of 768 —
//   1080p dense8x8 (1.26 MB frames)  16 384 frames 2941 / 2911 / 2874 us (-2.3 %), 8192: -2.1 %, 4096: -1.7 %, 2048: -1.6 %,
//                                    1024: 189.5 / 187.8 / 189.7, 768: 151.2 / 166.2 / 148.2, 512: 96.7 / 96.9 / 98.8 (+2.2 %)
//   720p dense8x8 (557 KB)           32 768 frames 2675 / 2659 / 2595 (-3.0 %)
// while smaller frames need the neighbours that stream during a workgroup's zeroing and cluster test —
//   1080p dense16 (316 KB)           65 536 frames 2923 / 2950 / 3116 (+6.6 %)
//   480p dense8x8 (186 KB)           1791 / 1762 / 1949;   720p dense16 (139 KB) 2632 / 2619 / 3284;   480p dense16 (46 KB,
//                                    8 per workgroup) 1765 / 1890 / 3204
//   compact records                  1080p dense8x8 (252 KB) 629 / 617 / 783, dense16 (63 KB) 691 / 824 / 1385
// (four per CU, which the kernels' SGPR count had never admitted, is slower than three: scan_kernels.hip).  So: one
// per CU for frames of half a megabyte and more, in launches that give every CU at least eight of them; two per CU
// gains 0.5-1.9 % on some of the shapes in between and loses 1-19 % on others: not taken.
constexpr int kLdsPerCu = 160 * 1024;
constexpr int kLdsOnePerCu = kLdsPerCu / 2 + 1024, kLdsTwoPerCu = kLdsPerCu / 3 + 1024;
int choose_lds_floor(const mtgpu_ctx *c, uint64_t n_records, uint32_t n_frames, int rec_bytes, int slices, int group) {
  int floor_bytes = 0;
  if (c->per_cu_request == 1) floor_bytes = kLdsOnePerCu;
  else if (c->per_cu_request == 2) floor_bytes = kLdsTwoPerCu;
  else if (c->per_cu_request == 0 && rec_bytes == MT_MV_BYTES && c->k.bands == 1 && slices == 1 && group == 1 && n_frames != 0) {
    const uint64_t avg = n_records * (uint64_t)rec_bytes / n_frames;
    const uint64_t cus = (uint64_t)(c->plan.cu_count > 0 ? c->plan.cu_count : 256);
    if (avg >= 512ull * 1024ull && (uint64_t)n_frames >= cus * 8ull) floor_bytes = kLdsOnePerCu;
  }
  return floor_bytes <= c->lds_max ? floor_bytes : 0;
}

// A scratch block of at least `bytes` for work queued on `st` (see mtgpu_ctx::Scratch).  The block is the caller's
// until scratch_release, which must follow the LAST launch that uses it.  Preference: a block that is large enough and
// whose last user has finished; an unused or small block to grow (small requests only); a block that is large enough
// but still in use (the stream then waits for it).  Growing synchronises with the block's last user and calls
// hipFree / hipMalloc: it happens while a context warms up, not in steady state.
int scratch_acquire(mtgpu_ctx *c, size_t bytes, hipStream_t st, int *slot_out, void **p_out) {
  using Scratch = mtgpu_ctx::Scratch;
  Scratch &sc = c->scratch;
  int pick = -1;
  {
    std::unique_lock<std::mutex> lock(sc.mu);
    for (;;) {
      // 1. a block this stream used last: stream order alone makes it safe, nothing to ask the runtime
      for (int i = 0; i < Scratch::kSlots && pick < 0; ++i) {
        const Scratch::Slot &s = sc.slot[i];
        if (!s.busy && s.cap >= bytes && s.recorded && s.last == st) pick = i;
      }
      // 2. a block that is large enough and whose last user has finished
      int fit_busy = -1, small_done = -1, small_busy = -1, unused = -1;
      for (int i = 0; i < Scratch::kSlots && pick < 0; ++i) {
        const Scratch::Slot &s = sc.slot[i];
        if (s.busy) continue;
        if (!s.recorded && s.cap >= bytes) { pick = i; break; }
        if (!s.recorded) { if (unused < 0 || s.cap > sc.slot[unused].cap) unused = i; continue; }
        const bool done = hipEventQuery(s.ev) == hipSuccess;
        if (s.cap >= bytes) { if (done) pick = i; else if (fit_busy < 0) fit_busy = i; }
        else if (done) { if (small_done < 0 || s.cap < sc.slot[small_done].cap) small_done = i; }
        else if (small_busy < 0) small_busy = i;
      }
      (void)hipGetLastError();                                  // (hipEventQuery's "not ready" is not an error of ours)
      // 3. small requests grow an idle block rather than wait; large ones (spill queues: gigabytes) wait for one that fits
      if (pick < 0 && bytes < Scratch::kBig) pick = unused >= 0 ? unused : small_done;
      if (pick < 0) pick = fit_busy;
      if (pick < 0) pick = unused >= 0 ? unused : (small_done >= 0 ? small_done : small_busy);
      if (pick >= 0) break;
      sc.cv.wait(lock);                                          // every block is in another thread's hands this microsecond
    }
    sc.slot[pick].busy = true;
  }
  mtgpu_ctx::Scratch::Slot &s = sc.slot[pick];
  hipError_t e = hipSuccess;
  if (!s.ev) e = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming);
  if (e == hipSuccess && s.cap < bytes) {
    if (s.recorded) e = hipEventSynchronize(s.ev);
    if (e == hipSuccess && s.p) { e = hipFree(s.p); s.p = nullptr; }
    const size_t old = s.cap;
    s.cap = 0;
    s.recorded = false;
    void *np = nullptr;
    const size_t want = bytes + bytes / 4 + 256;
    if (e == hipSuccess) e = hipMalloc(&np, want);
    if (e == hipSuccess) { s.p = np; s.cap = want; }
    std::lock_guard<std::mutex> lock(sc.mu);
    sc.reserved += s.cap;
    sc.reserved -= old;
    if (sc.reserved > sc.reserved_high) sc.reserved_high = sc.reserved;
  } else if (e == hipSuccess && s.recorded) {
    e = hipStreamWaitEvent(st, s.ev, 0);                        // after the block's last user, on whatever stream that was
  }
  if (e != hipSuccess) {
    { std::lock_guard<std::mutex> lock(sc.mu); s.busy = false; }
    sc.cv.notify_one();
    return hip_fail(e, "launch scratch");
  }
  *slot_out = pick;
  *p_out = s.p;
  return MT_OK;
}

// The caller has queued its last use of the block on `st`.
void scratch_release(mtgpu_ctx *c, int slot, hipStream_t st) {
  mtgpu_ctx::Scratch &sc = c->scratch;
  mtgpu_ctx::Scratch::Slot &s = sc.slot[slot];
  if (hipEventRecord(s.ev, st) == hipSuccess) {
    s.recorded = true;
    s.last = st;
  } else {                                                      // cannot tell when the work ends: wait for it here
    (void)hipGetLastError();
    (void)hipStreamSynchronize(st);
    s.recorded = false;
  }
  { std::lock_guard<std::mutex> lock(sc.mu); s.busy = false; }
  sc.cv.notify_one();
}

}  // namespace

#include "api_common.h"   // here: its helpers use mtgpu_ctx and the scratch ring above

namespace {

// Launches the scan on `st`; scratch (band centre counts, slice tiles + tickets) is allocated
// and freed stream-ordered, so concurrent callers share nothing.
// a caller's pointer (the *_device entry points): device memory takes plain stores; anything else the runtime
// knows of, or does not know at all, takes the system-scope ones
int result_memory_is_sys(const void *p) {
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof at);
  const hipError_t qe = hipPointerGetAttributes(&at, p);
  if (qe != hipSuccess) (void)hipGetLastError();        // only the failed query's own error is cleared
  return (qe == hipSuccess && at.type == hipMemoryTypeDevice) ? 0 : 1;
}

// flags_sys: 1 = d_flags is not device memory (system-scope result stores), 0 = device memory, -1 = ask the runtime
// d_centres (may be null; d_flags may be null when it is not) / centres_sys: the same for the frames' centre counts
int launch_scan_on(mtgpu_ctx *c, const void *d_mv, uint64_t n_records, const uint64_t *d_off,
                   const uint8_t *d_sd, uint32_t n_frames, uint8_t *d_flags, hipStream_t st, int rec_bytes = MT_MV_BYTES,
                   int flags_sys = 0, uint64_t rebase = 0, void *own_plan_ws = nullptr, size_t own_plan_ws_bytes = 0,
                   uint32_t *d_centres = nullptr, int centres_sys = 0) {
  if (flags_sys < 0) flags_sys = d_flags ? result_memory_is_sys(d_flags) : 0;
  if (centres_sys < 0) centres_sys = d_centres ? result_memory_is_sys(d_centres) : 0;
  mtgpu::ScanLaunch L;
  fill_batch(L, c, d_mv, rec_bytes, n_records, rebase, d_off, d_sd, n_frames, c->plan.lds_bytes, st);
  L.flags = d_flags;
  L.centres = d_centres;
  L.spill_q = nullptr;
  L.slice_ws = nullptr;
  L.tickets = nullptr;
  L.k = c->k;
  L.k.sys_flags = flags_sys;
  L.k.sys_centres = centres_sys;
  L.k.slices = choose_slices(c, n_records - rebase, n_frames);
  L.k.group = choose_group(c, n_records - rebase, n_frames, rec_bytes, L.k.slices);
  // the early exit: where the plan allows it (make_plan), on unsliced launches over 40-byte records that ask for the
  // flags alone — a centre count needs every record, a slice sees only its share of the votes — and that give every CU
  // at least eight frames (the bound of choose_lds_floor and choose_group: launches that fill the chip several times
  // over).  Every figure of the exit was taken there; a smaller launch reads each of its frames exactly once, as it
  // always did (its traffic is its algorithmic bytes), unless MTGPU_EARLY_EXIT=2 asks for the exit at any size.
  {
    const uint64_t cus = (uint64_t)(c->plan.cu_count > 0 ? c->plan.cu_count : 256);
    const bool large = c->early_exit == 2 || (uint64_t)n_frames >= cus * 8ull;
    L.k.early = (c->early_exit && large && rec_bytes == MT_MV_BYTES && L.k.bands == 1 && L.k.slices == 1 && L.k.fb == 32 &&
                 L.k.mode == 0 && L.k.vec_need >= 1u && L.k.clust_need <= 2u && d_flags != nullptr && d_centres == nullptr) ? 1 : 0;
  }
  if ((uint64_t)n_frames * (uint64_t)L.k.slices >= (1ull << 32))
    return fail(MT_ERR_INVALID, "%u frames x %d slices: work items must stay below 2^32 per call", n_frames, L.k.slices);
  L.block = c->plan.block_threads;
  L.item_chunk = (unsigned long long)c->item_chunk;
  if (c->wide_lds_bytes > c->plan.lds_bytes &&
      (uint64_t)n_frames * (uint64_t)L.k.bands * (uint64_t)L.k.slices <= (uint64_t)c->plan.cu_count) {
    L.k.chunk_rows = c->wide_chunk_rows;        // at most one workgroup per CU: bigger mask buffer, fewer chunks
    L.k.mask_rows = c->wide_chunk_rows + 2;
    L.lds_bytes = c->wide_lds_bytes;
  }
  // several frames per workgroup: their list entries are parked in LDS behind the tile (scan_kernels.hip, stage_items)
  L.k.stage_word = 0;
  if (L.k.group > 1) {
    const int at = (L.lds_bytes + 31) & ~31;
    if (at + mtgpu::kStageBytes <= c->lds_max) {
      L.k.stage_word = at / 4;
      L.lds_bytes = at + mtgpu::kStageBytes;
    } else {
      L.k.group = 1;                                          // a tile that fills LDS to the last 2 KB: one frame per workgroup
    }
  }
  // fewer workgroups per CU where that streams faster: the kernel never touches the LDS beyond its tile
  L.lds_bytes = std::max(L.lds_bytes, choose_lds_floor(c, n_records - rebase, n_frames, rec_bytes, L.k.slices, L.k.group));
  // launch scratch, one stream-ordered block: [work list + planning counts | spill queue or slice tiles + tickets]
  // the caller's own block for the work list (a pipe's batch), if it is large enough: the pool then serves only
  // the spill queue / the slice tiles, i.e. nothing at all for single-tile plans
  const bool own_plan = own_plan_ws && ((uintptr_t)own_plan_ws & 255u) == 0u && own_plan_ws_bytes >= mtgpu::plan_scratch_bytes(n_frames);
  const size_t plan_bytes = own_plan ? 0u : ((mtgpu::plan_scratch_bytes(n_frames) + 255u) & ~(size_t)255u);
  size_t bytes = plan_bytes;
  if (L.k.bands > 1) bytes += sizeof(unsigned int) * ((size_t)(n_records - rebase) + 4);   // spill queue: a slot per record
  if (L.k.slices > 1)
    bytes += sizeof(unsigned int) * ((size_t)n_frames * (size_t)L.k.slices * (size_t)L.k.cnt_words + (size_t)n_frames + 4);
  PlanWs ws(c, st, nullptr, bytes);
  if (ws.rc != MT_OK) return ws.rc;
  L.plan_ws = own_plan ? own_plan_ws : ws.p;
  unsigned int *rest = reinterpret_cast<unsigned int *>(static_cast<unsigned char *>(ws.p) + plan_bytes);
  if (L.k.bands > 1) L.spill_q = rest;
  if (L.k.slices > 1) {
    L.slice_ws = rest;
    L.tickets = L.slice_ws + (((size_t)n_frames * (size_t)L.k.slices * (size_t)L.k.cnt_words + 3) & ~(size_t)3);
  }
  return profiled_launch(c, st, L, mtgpu::launch_scan, "scan launch");
}

}  // namespace

namespace {
// MTGPU_ALIAS_DEVICES=N (tests, rehearsals on a box with fewer GPUs than the target node): the library presents N
// LOGICAL devices; logical device d runs on physical device d % (real count).  Everything above the C ABI — the
// host layer's stream -> device assignment, one shared context and scratch pool per (device, parameters), pipes
// per device — then takes its multi-device paths on a 1-GPU box.  Read once; 0 / unset = no aliasing.
int alias_devices() {
  static const int n = [] { const char *e = getenv("MTGPU_ALIAS_DEVICES"); return e ? std::max(0, atoi(e)) : 0; }();
  return n;
}
}  // namespace

namespace mtgpu {
// (the host copy-out loop, pack_records, lives in pack_simd.cpp: a plain host TU with per-CPU dispatch)
int ctx_device(const mtgpu_ctx *c) { return c->device; }
// A stream for one staging batch from the context's pool (created on first use of its slot; the caller has made
// the context's device current), or nullptr when the creation failed (the batch then creates a stream of its own).
hipStream_t ctx_pipe_stream(mtgpu_ctx *c) {
  std::lock_guard<std::mutex> lock(c->pipe_mu);
  const unsigned slot = c->pipe_rr++ % (unsigned)mtgpu_ctx::kMaxPipeStreams;
  if (!c->pipe_streams[slot] &&
      hipStreamCreateWithFlags(&c->pipe_streams[slot], hipStreamNonBlocking) != hipSuccess) {
    c->pipe_streams[slot] = nullptr;
    (void)hipGetLastError();
  }
  return c->pipe_streams[slot];
}
int physical_device(int logical) {
  int n = 0;
  if (alias_devices() <= 0 || hipGetDeviceCount(&n) != hipSuccess || n < 1) return logical;
  return logical >= 0 ? logical % n : logical;
}
int ctx_launch_scan(mtgpu_ctx *c, const void *d_mv, uint64_t n_records, const uint64_t *d_off,
                    const uint8_t *d_sd, uint32_t n_frames, uint8_t *d_flags, hipStream_t st, int rec_bytes, int flags_in_host_memory,
                    void *plan_ws, size_t plan_ws_bytes, uint32_t *d_centres) {
  return launch_scan_on(c, d_mv, n_records, d_off, d_sd, n_frames, d_flags, st, rec_bytes, flags_in_host_memory ? 1 : 0, 0,
                        plan_ws, plan_ws_bytes, d_centres, flags_in_host_memory ? 1 : 0);
}
size_t ctx_plan_ws_bytes(uint32_t n_frames) { return (plan_scratch_bytes(n_frames) + 255u) & ~(size_t)255u; }
}  // namespace mtgpu

#ifdef MTGPU_PHASE_TIMES
namespace mtgpu { hipError_t debug_set_phase_times(unsigned long long *p); }
extern "C" int mtgpu_debug_set_phase_times(void *p) {      // developer build only, not in include/mtgpu.h
  return mtgpu::debug_set_phase_times(static_cast<unsigned long long *>(p)) == hipSuccess ? MT_OK : MT_ERR_DEVICE;
}
#endif

extern "C" {

const char *mtgpu_version(void) {
  return "mtgpu 0.6 (gfx950 MV scan + segment merge)";
}

const char *mtgpu_last_error(void) { return g_err; }

int mtgpu_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  if (n > 0 && alias_devices() > 0) return alias_devices();
  return n;
}

int mtgpu_device_pci_address(int device, char *buf, uint64_t cap) {
  if (!buf) return fail(MT_ERR_INVALID, "buf is NULL");
  if (cap < 13) return fail(MT_ERR_CAPACITY, "buffer too small for a PCI address (13 bytes)");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(MT_ERR_DEVICE, "no HIP device available");
  const int logical = alias_devices() > 0 ? alias_devices() : n;
  if (device < 0 || device >= logical) return fail(MT_ERR_INVALID, "device %d outside [0,%d)", device, logical);
  char tmp[64] = "";
  hipError_t e = hipDeviceGetPCIBusId(tmp, (int)sizeof tmp, device % n);
  if (e != hipSuccess) return hip_fail(e, "hipDeviceGetPCIBusId");
  size_t i = 0;
  for (; tmp[i] && i + 1 < cap; ++i) buf[i] = (char)std::tolower((unsigned char)tmp[i]);
  buf[i] = 0;
  return MT_OK;
}

int mtgpu_params_from_config(mt_scan_params *out, int width, int height, double mv_threshold_sq,
                             int block_size, int block_shift, int vectors_needed,
                             int clusters_needed, float vertical_mask) {
  if (!out) return fail(MT_ERR_INVALID, "out is NULL");
  if (block_shift < 0 || block_shift > 31) return fail(MT_ERR_INVALID, "block_shift %d outside [0,31]", block_shift);
  // src/motion_scanner.cpp:190-193
  const long long gw = ((long long)width + block_size - 1) >> block_shift;
  const long long gh = ((long long)height + block_size - 1) >> block_shift;
  if (gw < 1 || gh < 1 || gw > 32767 || gh > 32767)
    return fail(MT_ERR_INVALID, "grid %lldx%lld outside [1,32767]", gw, gh);
  std::memset(out, 0, sizeof *out);
  out->mv_threshold_sq = mv_threshold_sq;              // :184
  out->block_shift = block_shift;                      // :185
  out->vectors_needed = (uint8_t)vectors_needed;       // :186, config.hpp:75
  out->clusters_needed = clusters_needed;              // :187
  out->grid_w = (int32_t)gw;
  out->grid_h = (int32_t)gh;
  const float margin = (float)(int16_t)gh * vertical_mask;   // :196, float32 product
  out->vertical_margin = (int)margin;
  return MT_OK;
}

int mtgpu_create(const mt_scan_params *params, int device, mtgpu_ctx **out) {
  if (!out) return fail(MT_ERR_INVALID, "out is NULL");
  *out = nullptr;
  int rc = validate_params(params);
  if (rc != MT_OK) return rc;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev < 1)
    return fail(MT_ERR_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  const int logical_devices = alias_devices() > 0 ? alias_devices() : ndev;
  if (device < 0 || device >= logical_devices) return fail(MT_ERR_INVALID, "device %d outside [0,%d)", device, logical_devices);
  const int logical = device;
  device = device % ndev;                    // (MTGPU_ALIAS_DEVICES: logical -> physical)
  HIP_TRY(hipSetDevice(device));
  int lds_max = 0, cus = 0;
  HIP_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  mtgpu_ctx *c = new (std::nothrow) mtgpu_ctx();
  if (!c) return fail(MT_ERR_NOMEM, "out of host memory");
  c->params = *params;
  c->device = device;
  c->logical_device = logical;
  c->lds_max = lds_max;
  c->stream = nullptr;
  rc = make_plan(c, lds_max, cus);
  if (rc != MT_OK) { delete c; return rc; }
  e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { delete c; return hip_fail(e, "hipStreamCreate"); }
  *out = c;
  return MT_OK;
}

void mtgpu_destroy(mtgpu_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
  for (hipStream_t &ps : c->pipe_streams)            // (pipes are destroyed before their context: include/mtgpu.h)
    if (ps) { (void)hipStreamSynchronize(ps); (void)hipStreamDestroy(ps); ps = nullptr; }
  for (auto &t : c->prof.ev)
    for (hipEvent_t &e : t)
      if (e) { (void)hipEventDestroy(e); e = nullptr; }
  for (auto &sl : c->scratch.slot) {
    if (sl.ev) { if (sl.recorded) (void)hipEventSynchronize(sl.ev); (void)hipEventDestroy(sl.ev); sl.ev = nullptr; }
    if (sl.p) { (void)hipFree(sl.p); sl.p = nullptr; }
  }
  c->d_mv.release(); c->d_off.release(); c->d_sd.release(); c->d_flags.release(); c->d_misc.release();
  delete c;
}

int mtgpu_get_stats(mtgpu_ctx *c, mtgpu_ctx_stats *out) {
  if (!c || !out) return fail(MT_ERR_INVALID, "NULL argument");
  std::memset(out, 0, sizeof *out);
  std::lock_guard<std::mutex> lock(c->mu);
  out->staging_device_bytes = c->d_mv.cap + c->d_off.cap + c->d_sd.cap + c->d_flags.cap + c->d_misc.cap;
  out->hip_streams = c->stream ? 1u : 0u;
  {
    std::lock_guard<std::mutex> pl(c->pipe_mu);
    for (hipStream_t ps : c->pipe_streams) out->hip_streams += ps ? 1u : 0u;
  }
  out->private_pool = 1u;
  {
    std::lock_guard<std::mutex> sl(c->scratch.mu);
    out->pool_reserved_bytes = c->scratch.reserved;
    out->pool_reserved_high = c->scratch.reserved_high;
  }
  return MT_OK;
}

int mtgpu_trim(mtgpu_ctx *c) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  // blocks nobody holds and whose last user has finished go back to the device; the others stay
  mtgpu_ctx::Scratch &sc = c->scratch;
  for (int i = 0; i < mtgpu_ctx::Scratch::kSlots; ++i) {
    mtgpu_ctx::Scratch::Slot &s = sc.slot[i];
    {
      std::lock_guard<std::mutex> lock(sc.mu);
      if (s.busy || !s.p) continue;
      if (s.recorded && hipEventQuery(s.ev) != hipSuccess) { (void)hipGetLastError(); continue; }
      s.busy = true;                                            // ours while it is being freed
    }
    const hipError_t e = hipFree(s.p);
    {
      std::lock_guard<std::mutex> lock(sc.mu);
      if (e == hipSuccess) { sc.reserved -= s.cap; s.p = nullptr; s.cap = 0; s.recorded = false; }
      s.busy = false;
    }
    sc.cv.notify_one();
    if (e != hipSuccess) return hip_fail(e, "hipFree(scratch)");
  }
  return MT_OK;
}

int mtgpu_get_params(const mtgpu_ctx *c, mt_scan_params *out) {
  if (!c || !out) return fail(MT_ERR_INVALID, "NULL argument");
  *out = c->params;
  return MT_OK;
}

int mtgpu_plan_preview(const mt_scan_params *params, int lds_bytes_per_workgroup, int cu_count, mtgpu_plan *out) {
  if (!out) return fail(MT_ERR_INVALID, "out is NULL");
  int rc = validate_params(params);
  if (rc != MT_OK) return rc;
  if (lds_bytes_per_workgroup < 1024 || cu_count < 1) return fail(MT_ERR_INVALID, "LDS size / CU count out of range");
  mtgpu_ctx *tmp = new (std::nothrow) mtgpu_ctx();          // host object only: no HIP call is made
  if (!tmp) return fail(MT_ERR_NOMEM, "out of host memory");
  tmp->params = *params;
  tmp->device = -1;
  tmp->logical_device = -1;
  tmp->stream = nullptr;
  tmp->lds_max = lds_bytes_per_workgroup;
  rc = make_plan(tmp, lds_bytes_per_workgroup, cu_count);
  if (rc == MT_OK) *out = tmp->plan;
  delete tmp;
  return rc;
}

int mtgpu_get_plan(const mtgpu_ctx *c, mtgpu_plan *out) {
  if (!c || !out) return fail(MT_ERR_INVALID, "NULL argument");
  *out = c->plan;
  return MT_OK;
}

namespace {
// MTGPU_CHECK_OFFSETS=1: verify the CSR precondition of the device entry points on the device, BEFORE the scan is
// queued — costs one small kernel and one stream synchronisation per call, which is why it is opt-in.
// Nothing unless the context asks for it and the batch has frames.
int check_offsets_on(mtgpu_ctx *c, const uint64_t *d_off, uint32_t n_frames, void *stream) {
  if (!c->check_offsets || n_frames == 0) return MT_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  PlanWs bad(c, st, nullptr, sizeof(unsigned int));
  if (bad.rc != MT_OK) return bad.rc;
  unsigned int first_bad = 0xffffffffu;
  hipError_t e = hipMemsetAsync(bad.p, 0xff, sizeof(unsigned int), st);
  if (e == hipSuccess)
    e = mtgpu::launch_check_offsets(reinterpret_cast<const unsigned long long *>(d_off), n_frames,
                                    static_cast<unsigned int *>(bad.p), st);
  if (e == hipSuccess) e = hipMemcpyAsync(&first_bad, bad.p, sizeof first_bad, hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail(e, "frame_off check");
  if (e2 != hipSuccess) return hip_fail(e2, "hipStreamSynchronize(frame_off check)");
  if (first_bad != 0xffffffffu)
    return fail(MT_ERR_INVALID, "frame_off[%u] > frame_off[%u]: record offsets must be non-decreasing "
                "(frames are disjoint record ranges; a banded plan keeps each frame's spill queue at its offset)",
                first_bad, first_bad + 1u);
  return MT_OK;
}
}  // namespace

int mtgpu_scan_frames_device(mtgpu_ctx *c, const void *d_mv, uint64_t n_records,
                             const uint64_t *d_frame_off, const uint8_t *d_has_sd,
                             uint32_t n_frames, uint8_t *d_flags, void *stream) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (n_frames == 0) return MT_OK;
  if (!d_frame_off || !d_flags) return fail(MT_ERR_INVALID, "frame_off/flags is NULL");
  if (n_records > 0 && !d_mv) return fail(MT_ERR_INVALID, "mv is NULL with n_records > 0");
  if (((uintptr_t)d_mv & 3u) != 0) return fail(MT_ERR_INVALID, "mv must be 4-byte aligned");
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_offsets_on(c, d_frame_off, n_frames, stream));
  return launch_scan_on(c, d_mv, n_records, d_frame_off, d_has_sd, n_frames, d_flags,
                        static_cast<hipStream_t>(stream), MT_MV_BYTES, -1);
}

int mtgpu_scan_frames_device_compact(mtgpu_ctx *c, const void *d_rec8, uint64_t n_records,
                                     const uint64_t *d_frame_off, const uint8_t *d_has_sd,
                                     uint32_t n_frames, uint8_t *d_flags, void *stream) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (n_frames == 0) return MT_OK;
  if (!d_frame_off || !d_flags) return fail(MT_ERR_INVALID, "frame_off/flags is NULL");
  if (n_records > 0 && !d_rec8) return fail(MT_ERR_INVALID, "records is NULL with n_records > 0");
  if (((uintptr_t)d_rec8 & 7u) != 0) return fail(MT_ERR_INVALID, "compact records must be 8-byte aligned");
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_offsets_on(c, d_frame_off, n_frames, stream));
  return launch_scan_on(c, d_rec8, n_records, d_frame_off, d_has_sd, n_frames, d_flags,
                        static_cast<hipStream_t>(stream), MT_COMPACT_BYTES, -1);
}

int mtgpu_scan_centres_device(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records,
                              const uint64_t *d_frame_off, const uint8_t *d_has_sd, uint32_t n_frames,
                              uint8_t *d_flags, uint32_t *d_centres, void *stream) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(check_rec_bytes(rec_bytes));
  if (n_frames == 0) return MT_OK;
  if (!d_frame_off) return fail(MT_ERR_INVALID, "frame_off is NULL");
  MT_TRY(check_any_output("d_", {{"flags", d_flags}, {"centres", d_centres}}));
  if (n_records > 0 && !d_rec) return fail(MT_ERR_INVALID, "d_rec is NULL with n_records > 0");
  MT_TRY(check_rec("d_", rec_bytes, d_rec));
  MT_TRY(check_aligned("d_", {{"centres", d_centres, 4}}));
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_offsets_on(c, d_frame_off, n_frames, stream));
  return launch_scan_on(c, d_rec, n_records, d_frame_off, d_has_sd, n_frames, d_flags, static_cast<hipStream_t>(stream),
                        rec_bytes, -1, 0, nullptr, 0, d_centres, -1);
}

int mtgpu_flags_from_centres_device(mtgpu_ctx *c, const uint32_t *d_centres, uint32_t n_frames, int32_t clusters_needed,
                                    uint8_t *d_flags, void *stream) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (n_frames == 0) return MT_OK;
  if (!d_centres || !d_flags) return fail(MT_ERR_INVALID, "d_centres/d_flags is NULL");
  HIP_TRY(hipSetDevice(c->device));
  const hipError_t e = mtgpu::launch_flags_from_centres(d_centres, n_frames, clusters_needed < 1 ? 1u : (unsigned int)clusters_needed,
                                                        d_flags, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "flags_from_centres launch");
  return MT_OK;
}

int mtgpu_pack_records(const void *mv_bytes, uint64_t n_records, void *out8) {
  if (n_records == 0) return MT_OK;
  if (!mv_bytes || !out8) return fail(MT_ERR_INVALID, "NULL argument");
  mtgpu::pack_records(static_cast<const unsigned char *>(mv_bytes), n_records, static_cast<unsigned char *>(out8));
  return MT_OK;
}

int mtgpu_pack_records_with(int impl_flags, const void *mv_bytes, uint64_t n_records, void *out8) {
  const int impl = impl_flags & MT_PACK_IMPL_MASK;
  if ((impl_flags & ~(MT_PACK_IMPL_MASK | MT_PACK_NT | MT_PACK_PREFETCH_LINES(255))) != 0 || impl < MT_PACK_SCALAR ||
      impl > MT_PACK_AVX512)
    return fail(MT_ERR_INVALID, "impl_flags must be MT_PACK_SCALAR, MT_PACK_AVX2 or MT_PACK_AVX512, optionally "
                "| MT_PACK_NT | MT_PACK_PREFETCH_LINES(0..255)");
  if (n_records > 0 && (!mv_bytes || !out8)) return fail(MT_ERR_INVALID, "NULL argument");
  const uint64_t prefetch = 64ull * (uint64_t)((impl_flags >> 8) & 255);
  if (mtgpu::pack_records_with(impl_flags & (MT_PACK_IMPL_MASK | MT_PACK_NT), static_cast<const unsigned char *>(mv_bytes),
                               n_records, static_cast<unsigned char *>(out8), prefetch) != 0)
    return fail(MT_ERR_UNSUPPORTED, "this CPU cannot run the requested copy-out loop");
  return MT_OK;
}

int mtgpu_pack_selected(void) { return mtgpu::pack_selected(); }

int mtgpu_profile_enable(mtgpu_ctx *c, int on) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  mtgpu_ctx::Profile &pf = c->prof;
  std::lock_guard<std::mutex> lock(pf.mu);
  if (on && !pf.created) {
    HIP_TRY(hipSetDevice(c->device));
    for (auto &t : pf.ev)
      for (hipEvent_t &e : t) HIP_TRY(hipEventCreate(&e));       // (a failure leaves what was created to mtgpu_destroy)
    pf.created = true;
  }
  pf.on.store(on ? 1 : 0, std::memory_order_relaxed);
  return MT_OK;
}

int mtgpu_profile_read(mtgpu_ctx *c, double *plan_ms, double *scan_ms, uint32_t *launches) {
  if (!c || !plan_ms || !scan_ms || !launches) return fail(MT_ERR_INVALID, "NULL argument");
  mtgpu_ctx::Profile &pf = c->prof;
  std::lock_guard<std::mutex> lock(pf.mu);
  while (pf.count > 0) {
    const hipError_t e = pf.drain_one();
    if (e != hipSuccess) return hip_fail(e, "profile events");
  }
  *plan_ms = pf.plan_ms; *scan_ms = pf.scan_ms; *launches = pf.launches;
  pf.plan_ms = pf.scan_ms = 0.0;
  pf.launches = 0;
  return MT_OK;
}

int mtgpu_set_slices(mtgpu_ctx *c, int slices) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (slices != 0 && slices != 1 && slices != 2 && slices != 4 && slices != 8)
    return fail(MT_ERR_INVALID, "slices must be 0 (auto), 1, 2, 4 or 8");
  c->slices_request.store(slices, std::memory_order_relaxed);
  return MT_OK;
}

}  // extern "C" (continued below)

namespace {
// mtgpu_scan_frames / mtgpu_scan_frames_centres: `flags` or `centres` may be NULL, not both (the callers checked)
int scan_frames_host(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off,
                     const uint8_t *has_sd, uint32_t n_frames, uint8_t *flags, uint32_t *centres) {
  for (uint32_t f = 0; f < n_frames; ++f)
    if (frame_off[f + 1] < frame_off[f])
      return fail(MT_ERR_INVALID, "frame_off not monotonic at frame %u", f);
  const uint64_t r_begin = frame_off[0], r_end = frame_off[n_frames];
  const uint64_t n_records = r_end - r_begin;
  if (n_records > 0 && !mv) return fail(MT_ERR_INVALID, "mv is NULL with records present");

  // d_flags: [flags n_frames | pad to 256 | centres n_frames x 4]; the flags' room stands with or without them
  Staged sg(c, c->d_flags, true, mv, r_begin, r_end, frame_off, has_sd, n_frames);
  const int o_fl = sg.out(flags, n_frames, true), o_cen = sg.out(centres, sizeof(uint32_t) * (size_t)n_frames);
  MT_TRY(sg.upload());
  MT_TRY(launch_scan_on(c, sg.d_mv(), r_end, sg.d_off(), sg.d_sd(), n_frames, sg.at<uint8_t>(o_fl), sg.st, MT_MV_BYTES, 0, r_begin,
                        nullptr, 0, sg.at<uint32_t>(o_cen), 0));
  return sg.download();
}
}  // namespace

extern "C" {

int mtgpu_scan_frames(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off,
                      const uint8_t *has_sd, uint32_t n_frames, uint8_t *flags) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (n_frames == 0) return MT_OK;
  if (!frame_off || !flags) return fail(MT_ERR_INVALID, "frame_off/flags is NULL");
  return scan_frames_host(c, mv, frame_off, has_sd, n_frames, flags, nullptr);
}

int mtgpu_scan_frames_centres(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off,
                              const uint8_t *has_sd, uint32_t n_frames, uint8_t *flags, uint32_t *centres) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (n_frames == 0) return MT_OK;
  if (!frame_off || !centres) return fail(MT_ERR_INVALID, "frame_off/centres is NULL");
  return scan_frames_host(c, mv, frame_off, has_sd, n_frames, flags, centres);
}

int mtgpu_merge_streams_device(mtgpu_ctx *c, const uint8_t *d_flags, const double *d_pts,
                               const uint64_t *d_stream_off, uint32_t n_streams,
                               const mt_merge_params *d_mp, int job_semantics, double *d_ts,
                               mt_segment *d_seg, uint64_t seg_cap, mt_merge_result *d_res,
                               void *stream) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (n_streams == 0) return MT_OK;
  if (!d_pts || !d_stream_off || !d_mp || !d_ts || !d_res || (seg_cap && !d_seg))
    return fail(MT_ERR_INVALID, "NULL device pointer");
  HIP_TRY(hipSetDevice(c->device));
  mtgpu::MergeLaunch L;
  L.flags = d_flags;
  L.pts = d_pts;
  L.stream_off = reinterpret_cast<const unsigned long long *>(d_stream_off);
  L.n_frames_total = ~0ull;   // stream_off is trusted to lie inside the caller's arrays
  L.mp = d_mp;
  L.job_semantics = job_semantics;
  L.ts_ws = d_ts;
  L.seg = d_seg;
  L.seg_cap = seg_cap;
  L.res = d_res;
  L.n_streams = n_streams;
  L.stream = static_cast<hipStream_t>(stream);
  hipError_t e = mtgpu::launch_merge(L);
  if (e != hipSuccess) return hip_fail(e, "merge launch");
  return MT_OK;
}

int mtgpu_sweep_streams_device(mtgpu_ctx *c, const uint32_t *d_centres, const double *d_pts,
                               const uint64_t *d_stream_off, uint32_t n_streams, uint64_t n_frames,
                               const mt_merge_params *d_mp, const int32_t *levels, uint32_t n_levels, int job_semantics,
                               double *d_ts, mt_segment *d_seg, uint64_t seg_cap, mt_merge_result *d_res,
                               void *stream) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (n_levels < 1 || n_levels > MT_SWEEP_MAX_LEVELS)
    return fail(MT_ERR_INVALID, "n_levels %u outside [1,%d]", n_levels, MT_SWEEP_MAX_LEVELS);
  if (!levels) return fail(MT_ERR_INVALID, "levels is NULL");
  if (n_streams == 0) return MT_OK;
  if (!d_centres || !d_pts || !d_stream_off || !d_mp || !d_ts || !d_res || (seg_cap && !d_seg))
    return fail(MT_ERR_INVALID, "NULL device pointer");
  HIP_TRY(hipSetDevice(c->device));
  mtgpu::MergeLaunch L;
  L.flags = nullptr;
  L.pts = d_pts;
  L.stream_off = reinterpret_cast<const unsigned long long *>(d_stream_off);
  L.n_frames_total = n_frames;          // the stride between the levels' workspaces; stream_off is clamped to it
  L.mp = d_mp;
  L.job_semantics = job_semantics;
  L.ts_ws = d_ts;
  L.seg = d_seg;
  L.seg_cap = seg_cap;
  L.res = d_res;
  L.n_streams = n_streams;
  L.stream = static_cast<hipStream_t>(stream);
  mtgpu::SweepLevels lv;
  for (uint32_t l = 0; l < MT_SWEEP_MAX_LEVELS; ++l)
    lv.need[l] = l < n_levels ? (levels[l] < 1 ? 1u : (unsigned int)levels[l]) : 0xffffffffu;   // :288 max(1, .)
  hipError_t e = mtgpu::launch_sweep(L, d_centres, lv, n_levels);
  if (e != hipSuccess) return hip_fail(e, "sweep launch");
  return MT_OK;
}

}  // extern "C" (continued below)

namespace {

// One stream's pooled timestamps, device-resident: small lists go to the one-workgroup stream
// kernel, large ones (>= merge_large_min) to the multi-workgroup path.  `ws` must hold
// merge_ts_ws_bytes(n); d_mp is ONE parameter block on the device.  Asynchronous on st.
size_t merge_ts_ws_bytes(const mtgpu_ctx *c, uint64_t n) {
  if (n >= c->merge_large_min && n > 0) return mtgpu::merge_large_ws_bytes(n);
  return sizeof(double) * 2 * (size_t)n + 64;          // [off[2] | pad] [ws 2n]
}

int merge_ts_on(mtgpu_ctx *c, const double *d_ts, uint64_t n, const mt_merge_params *d_mp, int job_semantics,
                void *ws, mt_segment *d_seg, uint64_t seg_cap, mt_merge_result *d_res, hipStream_t st) {
  if (n >= c->merge_large_min && n > 0) {
    hipError_t e = mtgpu::launch_merge_large(d_ts, n, d_mp, job_semantics, ws, d_seg, seg_cap, d_res, st);
    if (e != hipSuccess) return hip_fail(e, "large merge launch");
    return MT_OK;
  }
  unsigned char *w = static_cast<unsigned char *>(ws);
  mtgpu::MergeLaunch L;
  L.flags = nullptr;
  L.pts = d_ts;
  L.stream_off = nullptr;                               // one stream: [0, n)
  L.n_frames_total = n;
  L.mp = d_mp;
  L.job_semantics = job_semantics;
  L.ts_ws = reinterpret_cast<double *>(w + 64);
  L.seg = d_seg;
  L.seg_cap = seg_cap;
  L.res = d_res;
  L.n_streams = 1;
  L.stream = st;
  hipError_t e = mtgpu::launch_merge(L);
  if (e != hipSuccess) return hip_fail(e, "merge launch");
  return MT_OK;
}

}  // namespace

extern "C" {

int mtgpu_merge_timestamps_device(mtgpu_ctx *c, const double *d_ts, uint64_t n, const mt_merge_params *mp,
                                  int job_semantics, mt_segment *d_seg, uint64_t seg_cap,
                                  mt_merge_result *d_res, void *stream) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (!mp || !d_res) return fail(MT_ERR_INVALID, "mp/res is NULL");
  if (n > 0 && !d_ts) return fail(MT_ERR_INVALID, "ts is NULL with n > 0");
  if (seg_cap > 0 && !d_seg) return fail(MT_ERR_INVALID, "seg is NULL with seg_cap > 0");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t wsb = merge_ts_ws_bytes(c, n) + 64;               // + the parameter block
  PlanWs ws(c, st, nullptr, wsb);
  if (ws.rc != MT_OK) return ws.rc;
  unsigned char *w = static_cast<unsigned char *>(ws.p);
  hipError_t e = mtgpu::launch_store_params(*mp, reinterpret_cast<mt_merge_params *>(w), st);   // by value: captured now
  if (e != hipSuccess) return hip_fail(e, "merge params launch");
  return merge_ts_on(c, d_ts, n, reinterpret_cast<const mt_merge_params *>(w), job_semantics, w + 64, d_seg, seg_cap, d_res, st);
}

int mtgpu_merge_segments(mtgpu_ctx *c, const double *ts, uint64_t n, const mt_merge_params *mp,
                         int job_semantics, mt_segment *out, uint64_t cap, mt_merge_result *res) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (!mp || !res) return fail(MT_ERR_INVALID, "mp/res is NULL");
  if (n > 0 && !ts) return fail(MT_ERR_INVALID, "ts is NULL with n > 0");
  if (cap > 0 && !out) return fail(MT_ERR_INVALID, "out is NULL with cap > 0");

  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  // one staging block: mp | res | pts[n] | seg[segs] | workspace
  const uint64_t segs = (cap < n ? cap : n) + 1;        // K <= n; +1 for the full-copy segment
  size_t o_mp = 0;
  size_t o_res = o_mp + 64;
  size_t o_pts = o_res + 64;
  size_t o_seg = o_pts + sizeof(double) * (size_t)n;
  size_t o_ws = (o_seg + sizeof(mt_segment) * (size_t)segs + 63) & ~(size_t)63;
  size_t total = o_ws + merge_ts_ws_bytes(c, n);
  int rc = c->d_misc.reserve(total);
  if (rc != MT_OK) return rc;
  unsigned char *d = static_cast<unsigned char *>(c->d_misc.p);
  hipStream_t st = c->stream;
  DrainOnExit drain{st};
  if (n) HIP_TRY(hipMemcpyAsync(d + o_pts, ts, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d + o_mp, mp, sizeof *mp, hipMemcpyHostToDevice, st));
  rc = merge_ts_on(c, reinterpret_cast<const double *>(d + o_pts), n, reinterpret_cast<const mt_merge_params *>(d + o_mp),
                   job_semantics, d + o_ws, reinterpret_cast<mt_segment *>(d + o_seg), segs,
                   reinterpret_cast<mt_merge_result *>(d + o_res), st);
  if (rc != MT_OK) return rc;
  HIP_TRY(hipMemcpyAsync(res, d + o_res, sizeof *res, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (res->status != MT_OK) return fail(res->status, "timestamps contain NaN");
  const uint64_t ncopy = res->n_segments < cap ? res->n_segments : cap;
  if (ncopy) {
    HIP_TRY(hipMemcpyAsync(out, d + o_seg, sizeof(mt_segment) * (size_t)ncopy, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  if (res->n_segments > cap) return fail(MT_ERR_CAPACITY, "need %llu segments, capacity %llu",
                                         (unsigned long long)res->n_segments, (unsigned long long)cap);
  return MT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- motion scalar (tools/motion_scalar.cpp:61-84)

namespace {

// scores (+ terms) of a device-resident batch on `st`: launch scratch for the work list, the planner, the kernel.
// sys_*: 1 = the output is not device memory, 0 = device memory, -1 = ask the runtime
int motion_scores_on(mtgpu_ctx *c, const void *d_mv, uint64_t n_records, uint64_t rebase, const uint64_t *d_off,
                     uint32_t n_frames, double *d_scores, uint32_t *d_terms, hipStream_t st, int sys_scores, int sys_terms) {
  mtgpu::ScoresLaunch L;
  L.mv = static_cast<const unsigned char *>(d_mv);
  L.n_records = n_records;
  L.rebase = rebase;
  L.frame_off = reinterpret_cast<const unsigned long long *>(d_off);
  L.n_frames = n_frames;
  L.scores = d_scores;
  L.terms = d_terms;
  L.sys_scores = sys_scores < 0 ? result_memory_is_sys(d_scores) : sys_scores;
  L.sys_terms = d_terms ? (sys_terms < 0 ? result_memory_is_sys(d_terms) : sys_terms) : 0;
  L.stream = st;
  PlanWs ws(c, st, nullptr, mtgpu::ctx_plan_ws_bytes(n_frames));
  if (ws.rc != MT_OK) return ws.rc;
  L.plan_ws = ws.p;
  const hipError_t e = mtgpu::launch_motion_scores(L);
  if (e != hipSuccess) return hip_fail(e, "motion scores launch");
  return MT_OK;
}

int motion_bins_on(const double *d_scores, const uint32_t *d_terms, const double *d_pts, const uint64_t *d_stream_off,
                   uint32_t n_streams, uint32_t n_sec, double *d_acc, uint64_t *d_bin_terms, hipStream_t st, int sys_acc,
                   int sys_bin_terms) {
  mtgpu::BinsLaunch L;
  L.scores = d_scores;
  L.terms = d_terms;
  L.pts = d_pts;
  L.stream_off = reinterpret_cast<const unsigned long long *>(d_stream_off);
  L.n_streams = n_streams;
  L.n_sec = n_sec;
  L.acc = d_acc;
  L.bin_terms = reinterpret_cast<unsigned long long *>(d_bin_terms);
  L.sys_acc = sys_acc < 0 ? result_memory_is_sys(d_acc) : sys_acc;
  L.sys_bin_terms = d_bin_terms ? (sys_bin_terms < 0 ? result_memory_is_sys(d_bin_terms) : sys_bin_terms) : 0;
  L.stream = st;
  const hipError_t e = mtgpu::launch_motion_bins(L);
  if (e != hipSuccess) return hip_fail(e, "motion bins launch");
  return MT_OK;
}

}  // namespace

extern "C" {

int mtgpu_motion_scores_device(mtgpu_ctx *c, const void *d_mv, uint64_t n_records, const uint64_t *d_frame_off,
                               uint32_t n_frames, double *d_scores, uint32_t *d_terms, void *stream) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (n_frames == 0) return MT_OK;
  if (!d_frame_off || !d_scores) return fail(MT_ERR_INVALID, "d_frame_off/d_scores is NULL");
  if (n_records > 0 && !d_mv) return fail(MT_ERR_INVALID, "d_mv is NULL with n_records > 0");
  if (((uintptr_t)d_mv & 3u) != 0) return fail(MT_ERR_INVALID, "d_mv must be 4-byte aligned");
  if (((uintptr_t)d_scores & 7u) != 0) return fail(MT_ERR_INVALID, "d_scores must be 8-byte aligned");
  if (((uintptr_t)d_terms & 3u) != 0) return fail(MT_ERR_INVALID, "d_terms must be 4-byte aligned");
  HIP_TRY(hipSetDevice(c->device));
  return motion_scores_on(c, d_mv, n_records, 0, d_frame_off, n_frames, d_scores, d_terms, static_cast<hipStream_t>(stream),
                          -1, -1);
}

int mtgpu_motion_bins_device(mtgpu_ctx *c, const double *d_scores, const uint32_t *d_terms, const double *d_pts,
                             const uint64_t *d_stream_off, uint32_t n_streams, uint32_t n_sec, double *d_acc,
                             uint64_t *d_bin_terms, void *stream) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (n_sec == 0) return fail(MT_ERR_INVALID, "n_sec is 0");
  if (n_streams == 0) return MT_OK;
  if (!d_scores || !d_pts || !d_stream_off || !d_acc) return fail(MT_ERR_INVALID, "d_scores/d_pts/d_stream_off/d_acc is NULL");
  if (d_bin_terms && !d_terms) return fail(MT_ERR_INVALID, "d_bin_terms needs d_terms");
  if ((((uintptr_t)d_acc | (uintptr_t)d_bin_terms | (uintptr_t)d_scores | (uintptr_t)d_pts) & 7u) != 0)
    return fail(MT_ERR_INVALID, "d_scores, d_pts, d_acc and d_bin_terms must be 8-byte aligned");
  if (((uint64_t)n_sec + mtgpu::kBinsBlock - 1) / mtgpu::kBinsBlock * (uint64_t)n_streams >= (1ull << 31))
    return fail(MT_ERR_INVALID, "%u streams x %u seconds: too many bins for one call", n_streams, n_sec);
  HIP_TRY(hipSetDevice(c->device));
  return motion_bins_on(d_scores, d_terms, d_pts, d_stream_off, n_streams, n_sec, d_acc, d_bin_terms,
                        static_cast<hipStream_t>(stream), -1, -1);
}

int mtgpu_motion_scalar(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off, const double *pts, uint32_t n_frames,
                        uint32_t n_sec, double *acc, uint64_t *bin_terms) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (n_sec == 0) return fail(MT_ERR_INVALID, "n_sec is 0");
  if (!acc) return fail(MT_ERR_INVALID, "acc is NULL");
  if (n_frames > 0 && (!frame_off || !pts)) return fail(MT_ERR_INVALID, "frame_off/pts is NULL");
  for (uint32_t f = 0; f < n_frames; ++f)
    if (frame_off[f + 1] < frame_off[f]) return fail(MT_ERR_INVALID, "frame_off not monotonic at frame %u", f);
  const uint64_t r_begin = n_frames ? frame_off[0] : 0, r_end = n_frames ? frame_off[n_frames] : 0;
  const uint64_t n_records = r_end - r_begin;
  if (n_records > 0 && !mv) return fail(MT_ERR_INVALID, "mv is NULL with records present");

  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  int rc;
  if ((rc = c->d_mv.reserve((size_t)n_records * MT_MV_BYTES + 16)) != MT_OK) return rc;
  if ((rc = c->d_off.reserve(sizeof(uint64_t) * ((size_t)n_frames + 1))) != MT_OK) return rc;
  // one staging block: stream_off[2] | pts[F] | scores[F] | acc[n_sec] | bin_terms[n_sec] | terms[F]
  const size_t o_soff = 0, o_pts = 16, o_scores = o_pts + sizeof(double) * (size_t)n_frames;
  const size_t o_acc = o_scores + sizeof(double) * (size_t)n_frames, o_bt = o_acc + sizeof(double) * (size_t)n_sec;
  const size_t o_terms = o_bt + sizeof(uint64_t) * (size_t)n_sec, total = o_terms + sizeof(uint32_t) * (size_t)n_frames;
  if ((rc = c->d_misc.reserve(total)) != MT_OK) return rc;
  unsigned char *d = static_cast<unsigned char *>(c->d_misc.p);
  hipStream_t st = c->stream;
  DrainOnExit drain{st};
  const uint64_t soff[2] = {0, n_frames};
  HIP_TRY(hipMemcpyAsync(d + o_soff, soff, sizeof soff, hipMemcpyHostToDevice, st));
  if (n_frames) {
    if (n_records)
      HIP_TRY(hipMemcpyAsync(c->d_mv.p, mv + r_begin, (size_t)n_records * MT_MV_BYTES, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->d_off.p, frame_off, sizeof(uint64_t) * ((size_t)n_frames + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + o_pts, pts, sizeof(double) * (size_t)n_frames, hipMemcpyHostToDevice, st));
    // records of frame f live at d_mv + (frame_off[f] - r_begin) * 40: the work list is built with rebased offsets
    rc = motion_scores_on(c, c->d_mv.p, r_end, r_begin, static_cast<const uint64_t *>(c->d_off.p), n_frames,
                          reinterpret_cast<double *>(d + o_scores), reinterpret_cast<uint32_t *>(d + o_terms), st, 0, 0);
    if (rc != MT_OK) return rc;
  }
  rc = motion_bins_on(reinterpret_cast<const double *>(d + o_scores), reinterpret_cast<const uint32_t *>(d + o_terms),
                      reinterpret_cast<const double *>(d + o_pts), reinterpret_cast<const uint64_t *>(d + o_soff), 1, n_sec,
                      reinterpret_cast<double *>(d + o_acc), reinterpret_cast<uint64_t *>(d + o_bt), st, 0, 0);
  if (rc != MT_OK) return rc;
  HIP_TRY(hipMemcpyAsync(acc, d + o_acc, sizeof(double) * (size_t)n_sec, hipMemcpyDeviceToHost, st));
  if (bin_terms) HIP_TRY(hipMemcpyAsync(bin_terms, d + o_bt, sizeof(uint64_t) * (size_t)n_sec, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return MT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- setting sweep (src/motion_scanner.cpp:246-294 for every
// (MV_THRESHOLD_SQ, VECTORS_NEEDED) pair from one read of the records; include/mtgpu_sweep.h)

namespace {

static_assert(MT_SWEEP_MAX_THRESHOLDS == mtgpu::kSweepMaxThr && MT_SWEEP_MAX_VECTORS == mtgpu::kSweepMaxVec, "sweep limits");

// How the thresholds of a call are spread over launches for this grid and this much LDS: as many tiles per pass as
// fit next to a mask buffer of min(R, 8) + 2 rows (next to three rows if not even one tile fits that way), the passes
// balanced, and whatever room is left goes to the mask buffer.  *chunk_rows: centre rows per phase-2 chunk.
int sweep_plan(const mt_scan_params &p, int lds_max, uint32_t n_thr, uint32_t n_vec, mtgpu_sweep_plan *out, int *chunk_rows) {
  const int R = analysed_rows(p);
  const long long tile = (long long)mtgpu::sweep_tile_words(p.grid_w, R) * 4;
  const long long mask_row = (long long)((p.grid_w + 63) / 64) * 8 * (long long)n_vec;
  const long long fixed = (long long)mtgpu::kSweepMaxThr * mtgpu::kSweepMaxVec * 4;
  const auto fits = [&](long long n, long long rows) { return n * tile + (rows + 2) * mask_row + fixed <= (long long)lds_max; };
  if (!fits(1, 1))
    return fail(MT_ERR_UNSUPPORTED, "grid %dx%d: one tile of 32-bit counters for %d rows (%lld bytes) and a three-row mask buffer "
                "do not fit %d bytes of LDS; the sweep has no banded form (scan one setting per context instead)",
                p.grid_w, p.grid_h, R + 2, tile, lds_max);
  const long long want = R < 8 ? R : 8;
  long long fit = 0;
  for (long long n = n_thr; n >= 1 && fit == 0; --n) if (fits(n, want)) fit = n;
  for (long long n = n_thr; n >= 1 && fit == 0; --n) if (fits(n, 1)) fit = n;
  const long long passes = ((long long)n_thr + fit - 1) / fit, per = ((long long)n_thr + passes - 1) / passes;
  long long ch = ((long long)lds_max - per * tile - fixed) / mask_row - 2;
  if (ch > R) ch = R;
  out->thresholds_per_pass = (int32_t)per;
  out->passes = (int32_t)passes;
  out->lds_bytes = (int32_t)mtgpu::sweep_lds_bytes(p.grid_w, R, (int)per, (int)n_vec, (int)ch);
  out->counter_bits = 32;
  if (chunk_rows) *chunk_rows = (int)ch;
  return MT_OK;
}

int sweep_counts_ok(uint32_t n_thresholds, uint32_t n_vectors) {
  if (n_thresholds < 1 || n_thresholds > MT_SWEEP_MAX_THRESHOLDS)
    return fail(MT_ERR_INVALID, "n_thresholds %u outside [1,%d]", n_thresholds, MT_SWEEP_MAX_THRESHOLDS);
  if (n_vectors < 1 || n_vectors > MT_SWEEP_MAX_VECTORS)
    return fail(MT_ERR_INVALID, "n_vectors %u outside [1,%d]", n_vectors, MT_SWEEP_MAX_VECTORS);
  return MT_OK;
}

// The sweep of a device-resident batch on `st`: plan, launch scratch for the work list, the kernels.  The arguments
// have been validated.  centres_sys: 1 = the output is not device memory, 0 = device memory, -1 = ask the runtime
int sweep_on(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, uint64_t rebase, const uint64_t *d_off,
             const uint8_t *d_sd, uint32_t n_frames, const double *thresholds, uint32_t n_thr, const int32_t *vectors,
             uint32_t n_vec, uint32_t *d_centres, hipStream_t st, int centres_sys) {
  mtgpu_sweep_plan sp;
  int chunk_rows = 0;
  MT_TRY(sweep_plan(c->params, c->lds_max, n_thr, n_vec, &sp, &chunk_rows));
  mtgpu::SweepLaunch L;
  fill_batch(L, c, d_rec, rec_bytes, n_records, rebase, d_off, d_sd, n_frames, sp.lds_bytes, st);
  L.centres = d_centres;
  L.n_thr_all = (int)n_thr;
  L.thr_per_pass = sp.thresholds_per_pass;
  // ascending, as integers (stable: equal thresholds keep the caller's order; each gets a tile of its own)
  for (uint32_t i = 0; i < n_thr; ++i) {
    const unsigned long long t = threshold_to_int(thresholds[i]);
    uint32_t at = i;
    while (at > 0 && L.thr_sorted[at - 1] > t) { L.thr_sorted[at] = L.thr_sorted[at - 1]; L.thr_index[at] = L.thr_index[at - 1]; --at; }
    L.thr_sorted[at] = t;
    L.thr_index[at] = i;
  }
  for (uint32_t i = n_thr; i < (uint32_t)mtgpu::kSweepMaxThr; ++i) { L.thr_sorted[i] = ~0ull; L.thr_index[i] = 0u; }
  mtgpu::SweepK &k = L.k;
  fill_grid(k, c->k);
  for (uint32_t v = 0; v < (uint32_t)mtgpu::kSweepMaxVec; ++v)
    k.vec[v] = v < n_vec ? (unsigned int)(uint8_t)vectors[v] : 0xffffffffu;     // :186, config.hpp:75 — uint8
  k.n_vec = (int)n_vec;
  k.tile_words = (int)mtgpu::sweep_tile_words(k.gw, analysed_rows(c->params));
  k.chunk_rows = chunk_rows;
  k.mask_rows = chunk_rows + 2;
  k.sys = centres_sys < 0 ? result_memory_is_sys(d_centres) : centres_sys;
  PlanWs ws(c, st, nullptr, mtgpu::ctx_plan_ws_bytes(n_frames));
  if (ws.rc != MT_OK) return ws.rc;
  L.plan_ws = ws.p;
  return profiled_launch(c, st, L, mtgpu::launch_sweep_scan, "sweep scan launch");
}

}  // namespace

extern "C" {

int mtgpu_scan_sweep_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, uint32_t n_thresholds, uint32_t n_vectors,
                             mtgpu_sweep_plan *out) {
  if (!out) return fail(MT_ERR_INVALID, "out is NULL");
  MT_TRY(validate_params(p));
  if (lds_bytes_per_workgroup < 1024) return fail(MT_ERR_INVALID, "LDS size out of range");
  MT_TRY(sweep_counts_ok(n_thresholds, n_vectors));
  mtgpu_sweep_plan sp;
  MT_TRY(sweep_plan(*p, lds_bytes_per_workgroup, n_thresholds, n_vectors, &sp, nullptr));
  *out = sp;
  return MT_OK;
}

int mtgpu_scan_sweep_device(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, const uint64_t *d_frame_off,
                            const uint8_t *d_has_sd, uint32_t n_frames, const double *thresholds, uint32_t n_thresholds,
                            const int32_t *vectors, uint32_t n_vectors, uint32_t *d_centres, void *stream) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");      // the sweep, older than the rule below, asks for the context first
  MT_TRY(check_rec_bytes(rec_bytes));
  MT_TRY(sweep_counts_ok(n_thresholds, n_vectors));
  if (!thresholds) return fail(MT_ERR_INVALID, "thresholds is NULL");
  if (!vectors) return fail(MT_ERR_INVALID, "vectors is NULL");
  if (n_frames == 0) return MT_OK;
  if (!d_frame_off) return fail(MT_ERR_INVALID, "d_frame_off is NULL");
  if (!d_centres) return fail(MT_ERR_INVALID, "d_centres is NULL");
  if (n_records > 0 && !d_rec) return fail(MT_ERR_INVALID, "d_rec is NULL with n_records > 0");
  MT_TRY(check_rec("d_", rec_bytes, d_rec));
  MT_TRY(check_aligned("d_", {{"centres", d_centres, 4}}));
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_offsets_on(c, d_frame_off, n_frames, stream));
  return sweep_on(c, d_rec, rec_bytes, n_records, 0, d_frame_off, d_has_sd, n_frames, thresholds, n_thresholds, vectors,
                  n_vectors, d_centres, static_cast<hipStream_t>(stream), -1);
}

int mtgpu_scan_frames_sweep(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd, uint32_t n_frames,
                            const double *thresholds, uint32_t n_thresholds, const int32_t *vectors, uint32_t n_vectors,
                            uint32_t *centres) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");      // context first, as the device form
  MT_TRY(sweep_counts_ok(n_thresholds, n_vectors));
  if (!thresholds) return fail(MT_ERR_INVALID, "thresholds is NULL");
  if (!vectors) return fail(MT_ERR_INVALID, "vectors is NULL");
  if (n_frames == 0) return MT_OK;
  if (!frame_off || !centres) return fail(MT_ERR_INVALID, "frame_off/centres is NULL");
  MT_TRY(check_monotonic("frame_off", "frame", frame_off, n_frames));
  uint64_t r_begin, r_end;
  MT_TRY(check_window(mv, frame_off, n_frames, &r_begin, &r_end));
  {
    mtgpu_sweep_plan sp;                                   // a grid without a sweep form: before anything is staged
    MT_TRY(sweep_plan(c->params, c->lds_max, n_thresholds, n_vectors, &sp, nullptr));
  }
  Staged sg(c, c->d_flags, true, mv, r_begin, r_end, frame_off, has_sd, n_frames);
  const int o_cen = sg.out(centres, sizeof(uint32_t) * (size_t)n_thresholds * (size_t)n_vectors * (size_t)n_frames);
  MT_TRY(sg.upload());
  MT_TRY(sweep_on(c, sg.d_mv(), MT_MV_BYTES, r_end, r_begin, sg.d_off(), sg.d_sd(), n_frames, thresholds, n_thresholds, vectors,
                  n_vectors, sg.at<uint32_t>(o_cen), sg.st, 0));
  return sg.download();
}

}  // extern "C"

// ---------------------------------------------------------------- activity maps (src/motion_scanner.cpp:242-292 per frame,
// summed per stream and grid cell; include/mtgpu_activity.h)

namespace {

// Which form a grid gets with this much LDS: the tile, the frame's two mask planes, and two accumulator planes where
// they fit.  A workgroup has 1024 lanes, so at most two are resident per CU: accumulators that leave room for two
// workgroups are preferred over wider ones that do not (1080p: 16-bit fields, 61 KB, two per CU; 32-bit fields
// would take 90 KB and leave one).  Without room for 16-bit fields there are none and every frame flushes (4K).
int activity_plan(const mt_scan_params &p, int lds_max, mtgpu_activity_plan *out) {
  const int R = analysed_rows(p);
  const long long none = (long long)mtgpu::act_lds_bytes(p.grid_w, R, 0);
  const long long b16 = (long long)mtgpu::act_lds_bytes(p.grid_w, R, 16), b32 = (long long)mtgpu::act_lds_bytes(p.grid_w, R, 32);
  if (none > (long long)lds_max)
    return fail(MT_ERR_UNSUPPORTED, "grid %dx%d: one tile of 32-bit counters for %d rows and the frame's mask planes (%lld bytes) "
                "do not fit %d bytes of LDS; the activity map has no banded form", p.grid_w, p.grid_h, R + 2, none, lds_max);
  int bits = 0;
  if (2 * b32 <= (long long)lds_max) bits = 32;
  else if (2 * b16 <= (long long)lds_max) bits = 16;
  else if (b32 <= (long long)lds_max) bits = 32;
  else if (b16 <= (long long)lds_max) bits = 16;
  out->lds_bytes = (int32_t)(bits == 32 ? b32 : bits == 16 ? b16 : none);
  out->acc_bits = bits;
  out->max_run = bits == 32 ? 0x7fffffff : bits == 16 ? 65535 : 1;
  out->workgroup = mtgpu::kActBlock;
  return MT_OK;
}

// The map of a device-resident batch on `st`.  The arguments have been validated.
int activity_on(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, uint64_t rebase, const uint64_t *d_off,
                const uint8_t *d_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams, uint32_t min_centres,
                uint32_t run_frames, uint32_t *d_active, uint32_t *d_centre, uint32_t *d_frames, hipStream_t st) {
  mtgpu_activity_plan ap;
  MT_TRY(activity_plan(c->params, c->lds_max, &ap));
  mtgpu::ActLaunch L;
  fill_batch(L, c, d_rec, rec_bytes, n_records, rebase, d_off, d_sd, n_frames, ap.lds_bytes, st);
  L.stream_off = reinterpret_cast<const unsigned long long *>(d_stream_off);
  L.n_streams = n_streams;
  L.active = d_active; L.centre = d_centre; L.frames = d_frames;
  mtgpu::ActK &k = L.k;
  fill_tile(k, c->k, mtgpu::act_tile_words);
  k.min_centres = min_centres;
  k.gwp = mtgpu::act_gwp(k.gw);
  k.max_run = ap.max_run;
  {
    // the planner's run: about four rounds of workgroups on a chip that holds two per CU, at most 64 frames
    const uint64_t slots = 2u * (uint64_t)(c->plan.cu_count > 0 ? c->plan.cu_count : 256);
    uint64_t run = run_frames ? run_frames : (uint64_t)n_frames / (4u * slots);
    if (!run_frames && run > 64u) run = 64u;
    if (run < 1u) run = 1u;
    if (run > (uint64_t)ap.max_run) run = (uint64_t)ap.max_run;
    k.run = (int)run;
  }
  L.acc_bits = ap.acc_bits;
  if (n_frames == 0 || n_streams == 0) {                       // only the clear
    const hipError_t e = mtgpu::launch_activity_map(L);
    if (e != hipSuccess) return hip_fail(e, "activity map launch");
    return MT_OK;
  }
  PlanWs ws(c, st, nullptr, mtgpu::ctx_plan_ws_bytes(n_frames));
  if (ws.rc != MT_OK) return ws.rc;
  L.plan_ws = ws.p;
  return profiled_launch(c, st, L, mtgpu::launch_activity_map, "activity map launch");
}

}  // namespace

extern "C" {

int mtgpu_activity_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, mtgpu_activity_plan *out) {
  return preview(p, lds_bytes_per_workgroup, out, activity_plan);
}

int mtgpu_activity_map_device(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, const uint64_t *d_frame_off,
                              const uint8_t *d_has_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams,
                              uint32_t min_centres, uint32_t run_frames, uint32_t *d_active, uint32_t *d_centre,
                              uint32_t *d_frames, void *stream) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");      // context first, as the sweep
  MT_TRY(check_rec_bytes(rec_bytes));
  MT_TRY(check_any_output("d_", {{"active", d_active}, {"centre", d_centre}, {"frames", d_frames}}));
  if (n_frames > 0 && !d_frame_off) return fail(MT_ERR_INVALID, "d_frame_off is NULL");
  if (n_frames > 0 && n_streams > 0 && !d_stream_off) return fail(MT_ERR_INVALID, "d_stream_off is NULL");
  MT_TRY(check_aligned("d_", {{"frame_off", d_frame_off, 8}, {"stream_off", d_stream_off, 8}}));
  if (n_frames > 0 && n_records > 0 && !d_rec) return fail(MT_ERR_INVALID, "d_rec is NULL with n_records > 0");
  MT_TRY(check_rec("d_", rec_bytes, d_rec));
  MT_TRY(check_aligned("d_", {{"active", d_active, 4}, {"centre", d_centre, 4}, {"frames", d_frames, 4}}));
  MT_TRY(plan_ok(c, activity_plan));                         // a grid without a form: before any HIP call
  if (n_streams == 0) return MT_OK;                          // no stream owns an output element
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_on_device(c, {{"d_active", d_active}, {"d_centre", d_centre}, {"d_frames", d_frames}}, " (global atomics)"));
  MT_TRY(check_offsets_on(c, d_frame_off, n_frames, stream));
  return activity_on(c, d_rec, rec_bytes, n_records, 0, d_frame_off, d_has_sd, n_frames, d_stream_off, n_streams, min_centres,
                     run_frames, d_active, d_centre, d_frames, static_cast<hipStream_t>(stream));
}

int mtgpu_activity_map(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd, uint32_t n_frames,
                       const uint64_t *stream_off, uint32_t n_streams, uint32_t min_centres, uint32_t *active, uint32_t *centre,
                       uint32_t *frames) {
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");      // context first, as the sweep
  MT_TRY(check_any_output("", {{"active", active}, {"centre", centre}, {"frames", frames}}));
  if (!stream_off) return fail(MT_ERR_INVALID, "stream_off is NULL");
  if (n_frames > 0 && !frame_off) return fail(MT_ERR_INVALID, "frame_off is NULL");
  MT_TRY(check_monotonic("frame_off", "frame", frame_off, n_frames));
  MT_TRY(check_stream_off(stream_off, n_streams, n_frames));
  uint64_t r_begin, r_end;
  MT_TRY(check_window(mv, frame_off, n_frames, &r_begin, &r_end));
  MT_TRY(plan_ok(c, activity_plan));                         // a grid without a form: before anything is staged
  if (n_streams == 0) return MT_OK;

  // the room of `frames` stands whether it is asked for or not
  const size_t plane = sizeof(uint32_t) * (size_t)n_streams * (size_t)c->k.gh * (size_t)c->k.gw;
  Staged sg(c, c->d_misc, false, mv, r_begin, r_end, frame_off, has_sd, n_frames);
  const int i_soff = sg.in(stream_off, sizeof(uint64_t) * ((size_t)n_streams + 1));
  const int o_act = sg.out(active, plane), o_cen = sg.out(centre, plane), o_fr = sg.out(frames, sizeof(uint32_t) * (size_t)n_streams, true);
  MT_TRY(sg.upload());
  MT_TRY(activity_on(c, sg.d_mv(), MT_MV_BYTES, r_end, r_begin, sg.d_off(), sg.d_sd(), n_frames, sg.at<const uint64_t>(i_soff),
                     n_streams, min_centres, 0, sg.at<uint32_t>(o_act), sg.at<uint32_t>(o_cen), sg.at<uint32_t>(o_fr), sg.st));
  return sg.download();
}

}  // extern "C"

// ---------------------------------------------------------------- ignore zones (src/motion_scanner.cpp:242-292 per frame,
// :282 ANDed with a per-stream keep bit; include/mtgpu_zones.h)

namespace {

// One form: the tile, the staged keep rows and two mask planes.  It fits or the grid is unsupported.
int zones_plan(const mt_scan_params &p, int lds_max, mtgpu_zones_plan *out) {
  const int R = analysed_rows(p);
  const long long need = (long long)mtgpu::zone_lds_bytes(p.grid_w, R);
  if (need > (long long)lds_max)
    return fail(MT_ERR_UNSUPPORTED, "grid %dx%d: one tile of 32-bit counters for %d rows, the keep rows and two mask planes "
                "(%lld bytes) do not fit %d bytes of LDS; the masked scan has no banded form", p.grid_w, p.grid_h, R + 2, need, lds_max);
  const long long W = ((long long)p.grid_w + 63) / 64;
  out->lds_bytes = (int32_t)need;
  out->workgroup = mtgpu::kZoneBlock;
  out->keep_words_per_row = (int32_t)W;
  out->keep_words_per_stream = (int32_t)(W * (long long)p.grid_h);
  return MT_OK;
}

// The masked scan of a device-resident batch on `st`.  The arguments have been validated; n_frames > 0.
// own_plan_ws: the caller's own block for the work list (a pipe's batch; ctx_plan_ws_bytes(n_frames) bytes, 256-byte
// aligned) — the launch then takes NOTHING from the context's scratch ring — and the pipe form of the launch: one plane,
// no clear kernel, outputs stored at system scope when `outputs_in_host_memory`.  nullptr: the ring, the stream form.
int zones_on(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, uint64_t rebase, const uint64_t *d_off,
             const uint8_t *d_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams, const uint64_t *d_keep,
             uint8_t *d_flags, uint32_t *d_centres, uint32_t *d_centres_all, hipStream_t st, void *own_plan_ws = nullptr,
             int outputs_in_host_memory = 0) {
  mtgpu_zones_plan zp;
  MT_TRY(zones_plan(c->params, c->lds_max, &zp));
  mtgpu::ZoneLaunch L;
  fill_batch(L, c, d_rec, rec_bytes, n_records, rebase, d_off, d_sd, n_frames, zp.lds_bytes, st);
  L.stream_off = reinterpret_cast<const unsigned long long *>(d_stream_off);
  L.n_streams = n_streams;
  L.keep = reinterpret_cast<const unsigned long long *>(d_keep);
  L.flags = d_flags; L.centres = d_centres; L.centres_all = d_centres_all;
  fill_tile(L.k, c->k, mtgpu::zone_tile_words);
  L.k.clust_need = c->k.clust_need;
  if (own_plan_ws) {
    L.pipe = 1;
    L.sys_flags = (d_flags && outputs_in_host_memory) ? 1 : 0;
    L.sys_centres = (d_centres && outputs_in_host_memory) ? 1 : 0;
  }
  PlanWs ws(c, st, own_plan_ws, mtgpu::ctx_plan_ws_bytes(n_frames));
  if (ws.rc != MT_OK) return ws.rc;
  L.plan_ws = ws.p;
  return profiled_launch(c, st, L, mtgpu::launch_zone_scan, "zone scan launch");
}

}  // namespace

namespace mtgpu {
int ctx_zones_keep_words(const mtgpu_ctx *c, uint64_t *words) {
  mtgpu_zones_plan zp;
  MT_TRY(zones_plan(c->params, c->lds_max, &zp));
  *words = (uint64_t)zp.keep_words_per_stream;
  return MT_OK;
}
int ctx_launch_zones(mtgpu_ctx *c, const void *d_rec, uint64_t n_records, const uint64_t *d_off, const uint8_t *d_sd,
                     uint32_t n_frames, const uint64_t *d_keep, uint8_t *d_flags, uint32_t *d_centres, hipStream_t st, int rec_bytes,
                     int outputs_in_host_memory, void *plan_ws, size_t plan_ws_bytes) {
  if (n_frames == 0) return MT_OK;
  if (!d_keep) return fail(MT_ERR_INVALID, "masked pipe scan without a keep plane");
  MT_TRY(check_pipe_ws("masked", plan_ws, plan_ws_bytes, n_frames));
  return zones_on(c, d_rec, rec_bytes, n_records, 0, d_off, d_sd, n_frames, nullptr, 1, d_keep, d_flags, d_centres, nullptr, st,
                  plan_ws, outputs_in_host_memory ? 1 : 0);
}
}  // namespace mtgpu

extern "C" {

int mtgpu_zones_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, mtgpu_zones_plan *out) {
  return preview(p, lds_bytes_per_workgroup, out, zones_plan);
}

int mtgpu_scan_zones_device(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, const uint64_t *d_frame_off,
                            const uint8_t *d_has_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams,
                            const uint64_t *d_keep, uint8_t *d_flags, uint32_t *d_centres, uint32_t *d_centres_all, void *stream) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(check_rec_bytes(rec_bytes));
  MT_TRY(check_any_output("d_", {{"flags", d_flags}, {"centres", d_centres}, {"centres_all", d_centres_all}}));
  if (n_frames > 0 && !d_frame_off) return fail(MT_ERR_INVALID, "d_frame_off is NULL");
  // the stream table and the keep planes are REQUIRED here, and only a batch with frames is asked for them
  if (n_frames > 0 && n_streams == 0) return fail(MT_ERR_INVALID, "n_streams is 0 with n_frames > 0");
  if (n_frames > 0 && !d_stream_off) return fail(MT_ERR_INVALID, "d_stream_off is NULL");
  if (n_frames > 0 && !d_keep) return fail(MT_ERR_INVALID, "d_keep is NULL");
  MT_TRY(check_aligned("d_", {{"frame_off", d_frame_off, 8}, {"stream_off", d_stream_off, 8}, {"keep", d_keep, 8}}));
  if (n_frames > 0 && n_records > 0 && !d_rec) return fail(MT_ERR_INVALID, "d_rec is NULL with n_records > 0");
  MT_TRY(check_rec("d_", rec_bytes, d_rec));
  MT_TRY(check_aligned("d_", {{"centres", d_centres, 4}, {"centres_all", d_centres_all, 4}}));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(plan_ok(c, zones_plan));                            // a grid without a form: before any HIP call
  if (n_frames == 0) return MT_OK;
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_on_device(c, {{"d_keep", d_keep}, {"d_flags", d_flags}, {"d_centres", d_centres}, {"d_centres_all", d_centres_all}}));
  MT_TRY(check_offsets_on(c, d_frame_off, n_frames, stream));
  return zones_on(c, d_rec, rec_bytes, n_records, 0, d_frame_off, d_has_sd, n_frames, d_stream_off, n_streams, d_keep, d_flags,
                  d_centres, d_centres_all, static_cast<hipStream_t>(stream));
}

int mtgpu_scan_frames_zones(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd, uint32_t n_frames,
                            const uint64_t *stream_off, uint32_t n_streams, const uint64_t *keep, uint8_t *flags,
                            uint32_t *centres, uint32_t *centres_all) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(check_any_output("", {{"flags", flags}, {"centres", centres}, {"centres_all", centres_all}}));
  // the host form reads stream_off[n_streams] whatever n_frames is: it asks for the table ahead of frame_off
  if (!stream_off) return fail(MT_ERR_INVALID, "stream_off is NULL");
  if (n_frames > 0 && !frame_off) return fail(MT_ERR_INVALID, "frame_off is NULL");
  if (n_frames > 0 && n_streams == 0) return fail(MT_ERR_INVALID, "n_streams is 0 with n_frames > 0");
  if (n_frames > 0 && !keep) return fail(MT_ERR_INVALID, "keep is NULL");
  MT_TRY(check_monotonic("frame_off", "frame", frame_off, n_frames));
  MT_TRY(check_stream_off(stream_off, n_streams, n_frames));
  uint64_t r_begin, r_end;
  MT_TRY(check_window(mv, frame_off, n_frames, &r_begin, &r_end));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(plan_ok(c, zones_plan));                            // a grid without a form: before anything is staged
  if (n_frames == 0) return MT_OK;

  const size_t words = sizeof(uint32_t) * (size_t)n_frames;
  Staged sg(c, c->d_misc, false, mv, r_begin, r_end, frame_off, has_sd, n_frames);
  const int i_soff = sg.in(stream_off, sizeof(uint64_t) * ((size_t)n_streams + 1));
  const int i_keep = sg.in(keep, sizeof(uint64_t) * (size_t)n_streams * (size_t)c->k.gh * (size_t)c->k.W);
  const int o_fl = sg.out(flags, n_frames), o_cen = sg.out(centres, words), o_all = sg.out(centres_all, words);
  MT_TRY(sg.upload());
  MT_TRY(zones_on(c, sg.d_mv(), MT_MV_BYTES, r_end, r_begin, sg.d_off(), sg.d_sd(), n_frames, sg.at<const uint64_t>(i_soff), n_streams,
                  sg.at<const uint64_t>(i_keep), sg.at<uint8_t>(o_fl), sg.at<uint32_t>(o_cen), sg.at<uint32_t>(o_all), sg.st));
  return sg.download();
}

}  // extern "C"

// ---------------------------------------------------------------- motion blobs (src/motion_scanner.cpp:272-294 per frame,
// then the connected components of the centres; include/mtgpu_blobs.h)

namespace {

static_assert(sizeof(mt_blob_box) == sizeof(mtgpu::BlobBox) && sizeof(mt_blob_box) == 8, "mt_blob_box is four uint16");

// One form: the tile (the labels later), the staged keep rows (the centre plane later) and one mask plane.
int blobs_plan(const mt_scan_params &p, int lds_max, mtgpu_blobs_plan *out) {
  const int R = analysed_rows(p);
  const long long need = (long long)mtgpu::blob_lds_bytes(p.grid_w, R);
  if (need > (long long)lds_max)
    return fail(MT_ERR_UNSUPPORTED, "grid %dx%d: one tile of 32-bit counters for %d rows, the keep rows and one mask plane "
                "(%lld bytes) do not fit %d bytes of LDS; the blob scan has no banded form", p.grid_w, p.grid_h, R + 2, need, lds_max);
  const long long W = ((long long)p.grid_w + 63) / 64;
  out->lds_bytes = (int32_t)need;
  out->workgroup = mtgpu::kBlobBlock;
  out->keep_words_per_row = (int32_t)W;
  out->keep_words_per_stream = (int32_t)(W * (long long)p.grid_h);
  return MT_OK;
}

// The blob scan of a device-resident batch on `st`.  The arguments have been validated; n_frames > 0.
// own_plan_ws: the caller's own block for the work list (a pipe's batch; ctx_plan_ws_bytes(n_frames) bytes, 256-byte
// aligned) — the launch then takes NOTHING from the context's scratch ring — and the pipe form of the launch: one plane
// or none, no clear kernel, flags and one count stored at system scope when `outputs_in_host_memory`.  nullptr: the
// ring, the stream form.
int blobs_on(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, uint64_t rebase, const uint64_t *d_off,
             const uint8_t *d_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams, const uint64_t *d_keep,
             int32_t min_blob_cells, uint8_t *d_flags, uint32_t *d_centres, uint32_t *d_blobs, uint32_t *d_largest,
             mt_blob_box *d_box, hipStream_t st, void *own_plan_ws = nullptr, int outputs_in_host_memory = 0) {
  mtgpu_blobs_plan bp;
  MT_TRY(blobs_plan(c->params, c->lds_max, &bp));
  mtgpu::BlobLaunch L;
  fill_batch(L, c, d_rec, rec_bytes, n_records, rebase, d_off, d_sd, n_frames, bp.lds_bytes, st);
  L.stream_off = reinterpret_cast<const unsigned long long *>(d_stream_off);
  L.n_streams = n_streams;
  L.keep = reinterpret_cast<const unsigned long long *>(d_keep);
  L.flags = d_flags; L.centres = d_centres; L.blobs = d_blobs; L.largest = d_largest;
  L.box = reinterpret_cast<mtgpu::BlobBox *>(d_box);
  fill_tile(L.k, c->k, mtgpu::blob_tile_words);
  L.k.clust_need = c->k.clust_need;
  L.k.blob_need = min_blob_cells < 1 ? 1u : (unsigned int)min_blob_cells;
  if (own_plan_ws) {
    L.pipe = 1;
    L.sys_flags = (d_flags && outputs_in_host_memory) ? 1 : 0;
    L.sys_centres = ((d_centres || d_largest) && outputs_in_host_memory) ? 1 : 0;
  }
  PlanWs ws(c, st, own_plan_ws, mtgpu::ctx_plan_ws_bytes(n_frames));
  if (ws.rc != MT_OK) return ws.rc;
  L.plan_ws = ws.p;
  return profiled_launch(c, st, L, mtgpu::launch_blob_scan, "blob scan launch");
}

}  // namespace

namespace mtgpu {
int ctx_blobs_supported(const mtgpu_ctx *c) { return plan_ok(c, blobs_plan); }
int ctx_launch_blobs(mtgpu_ctx *c, const void *d_rec, uint64_t n_records, const uint64_t *d_off, const uint8_t *d_sd,
                     uint32_t n_frames, const uint64_t *d_keep, int32_t min_blob_cells, int report_largest, uint8_t *d_flags,
                     uint32_t *d_count, hipStream_t st, int rec_bytes, int outputs_in_host_memory, void *plan_ws,
                     size_t plan_ws_bytes, mt_blob_box *d_box) {
  if (n_frames == 0) return MT_OK;
  if (min_blob_cells < 1) return fail(MT_ERR_INVALID, "blob pipe scan with min_blob_cells %d", (int)min_blob_cells);
  MT_TRY(check_pipe_ws("blob", plan_ws, plan_ws_bytes, n_frames));
  // the boxed kernel stores a box as ONE 64-bit word: 8-byte aligned here, against 2 in mtgpu_scan_blobs_device
  if (((uintptr_t)d_box & 7u) != 0u) return fail(MT_ERR_INVALID, "blob pipe scan: the batch's box array must be 8-byte aligned");
  return blobs_on(c, d_rec, rec_bytes, n_records, 0, d_off, d_sd, n_frames, nullptr, 0, d_keep, min_blob_cells, d_flags,
                  report_largest ? nullptr : d_count, nullptr, report_largest ? d_count : nullptr, d_box, st, plan_ws,
                  outputs_in_host_memory ? 1 : 0);
}
}  // namespace mtgpu

extern "C" {

int mtgpu_blobs_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, mtgpu_blobs_plan *out) {
  return preview(p, lds_bytes_per_workgroup, out, blobs_plan);
}

int mtgpu_scan_blobs_device(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, const uint64_t *d_frame_off,
                            const uint8_t *d_has_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams,
                            const uint64_t *d_keep, int32_t min_blob_cells, uint8_t *d_flags, uint32_t *d_centres,
                            uint32_t *d_blobs, uint32_t *d_largest, mt_blob_box *d_box, void *stream) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(check_rec_bytes(rec_bytes));
  MT_TRY(check_any_output("d_", {{"flags", d_flags}, {"centres", d_centres}, {"blobs", d_blobs}, {"largest", d_largest}, {"box", d_box}}));
  if (n_frames > 0 && !d_frame_off) return fail(MT_ERR_INVALID, "d_frame_off is NULL");
  MT_TRY(check_stream_table("d_", d_stream_off, n_streams, d_keep));
  MT_TRY(check_aligned("d_", {{"frame_off", d_frame_off, 8}, {"stream_off", d_stream_off, 8}, {"keep", d_keep, 8}}));
  if (n_frames > 0 && n_records > 0 && !d_rec) return fail(MT_ERR_INVALID, "d_rec is NULL with n_records > 0");
  MT_TRY(check_rec("d_", rec_bytes, d_rec));
  // (four 16-bit stores per box here: 2-byte aligned, against 8 in the pipe doorway)
  MT_TRY(check_aligned("d_", {{"centres", d_centres, 4}, {"blobs", d_blobs, 4}, {"largest", d_largest, 4}, {"box", d_box, 2}}));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(plan_ok(c, blobs_plan));                            // a grid without a form: before any HIP call
  if (n_frames == 0) return MT_OK;
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_on_device(c, {{"d_keep", d_keep}, {"d_flags", d_flags}, {"d_centres", d_centres}, {"d_blobs", d_blobs},
                             {"d_largest", d_largest}, {"d_box", d_box}}));
  MT_TRY(check_offsets_on(c, d_frame_off, n_frames, stream));
  return blobs_on(c, d_rec, rec_bytes, n_records, 0, d_frame_off, d_has_sd, n_frames, d_stream_off, n_streams, d_keep,
                  min_blob_cells, d_flags, d_centres, d_blobs, d_largest, d_box, static_cast<hipStream_t>(stream));
}

int mtgpu_scan_frames_blobs(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd, uint32_t n_frames,
                            const uint64_t *stream_off, uint32_t n_streams, const uint64_t *keep, int32_t min_blob_cells,
                            uint8_t *flags, uint32_t *centres, uint32_t *blobs, uint32_t *largest, mt_blob_box *box) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(check_any_output("", {{"flags", flags}, {"centres", centres}, {"blobs", blobs}, {"largest", largest}, {"box", box}}));
  if (n_frames > 0 && !frame_off) return fail(MT_ERR_INVALID, "frame_off is NULL");
  MT_TRY(check_stream_table("", stream_off, n_streams, keep));
  MT_TRY(check_monotonic("frame_off", "frame", frame_off, n_frames));
  if (keep) MT_TRY(check_stream_off(stream_off, n_streams, n_frames));
  uint64_t r_begin, r_end;
  MT_TRY(check_window(mv, frame_off, n_frames, &r_begin, &r_end));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(plan_ok(c, blobs_plan));                            // a grid without a form: before anything is staged
  if (n_frames == 0) return MT_OK;

  // (without a mask stream_off and keep are null and n_streams is 0: no room, null device pointers)
  const size_t words = sizeof(uint32_t) * (size_t)n_frames;
  Staged sg(c, c->d_misc, false, mv, r_begin, r_end, frame_off, has_sd, n_frames);
  const int i_soff = sg.in(stream_off, sizeof(uint64_t) * ((size_t)n_streams + 1));
  const int i_keep = sg.in(keep, sizeof(uint64_t) * (size_t)n_streams * (size_t)c->k.gh * (size_t)c->k.W);
  const int o_fl = sg.out(flags, n_frames), o_cen = sg.out(centres, words), o_bl = sg.out(blobs, words), o_lg = sg.out(largest, words);
  const int o_box = sg.out(box, sizeof(mt_blob_box) * (size_t)n_frames);
  MT_TRY(sg.upload());
  MT_TRY(blobs_on(c, sg.d_mv(), MT_MV_BYTES, r_end, r_begin, sg.d_off(), sg.d_sd(), n_frames, sg.at<const uint64_t>(i_soff), n_streams,
                  sg.at<const uint64_t>(i_keep), min_blob_cells, sg.at<uint8_t>(o_fl), sg.at<uint32_t>(o_cen), sg.at<uint32_t>(o_bl),
                  sg.at<uint32_t>(o_lg), sg.at<mt_blob_box>(o_box), sg.st));
  return sg.download();
}

}  // extern "C"

// ---------------------------------------------------------------- global-motion compensation (src/motion_scanner.cpp:242-292
// per frame, :246-251 on the residuals of the frame's dominant vector; include/mtgpu_gmc.h)

namespace {

static_assert(sizeof(mt_gmc_info) == 4u * mtgpu::kGmcInfoWords && alignof(mt_gmc_info) == 4, "mt_gmc_info is five 32-bit words");
static_assert(MTGPU_GMC_MAX_SHIFT == mtgpu::kGmcMaxShift && 2 * mtgpu::kGmcMaxShift + 1 <= mtgpu::kGmcHistBins, "histogram bins");

// One form: the tile, one mask plane and the two histograms.  It fits or the grid is unsupported.
int gmc_plan(const mt_scan_params &p, int lds_max, mtgpu_gmc_plan *out) {
  const int R = analysed_rows(p);
  const long long need = (long long)mtgpu::gmc_lds_bytes(p.grid_w, R);
  if (need > (long long)lds_max)
    return fail(MT_ERR_UNSUPPORTED, "grid %dx%d: one tile of 32-bit counters for %d rows, one mask plane and the histograms "
                "(%lld bytes) do not fit %d bytes of LDS; the compensated scan has no banded form", p.grid_w, p.grid_h, R + 2, need, lds_max);
  out->lds_bytes = (int32_t)need;
  out->workgroup = mtgpu::kGmcBlock;
  out->hist_bins = mtgpu::kGmcHistBins;
  out->info_bytes = (int32_t)sizeof(mt_gmc_info);
  return MT_OK;
}

// What max_shift and min_share_q8 alone decide.
int gmc_check_settings(int32_t max_shift, int32_t min_share_q8) {
  if (max_shift < 0 || max_shift > MTGPU_GMC_MAX_SHIFT)
    return fail(MT_ERR_INVALID, "max_shift must be in [0, %d], not %d", MTGPU_GMC_MAX_SHIFT, (int)max_shift);
  if (min_share_q8 < 0 || min_share_q8 > 256) return fail(MT_ERR_INVALID, "min_share_q8 must be in [0, 256], not %d", (int)min_share_q8);
  return MT_OK;
}

// The compensated scan of a device-resident batch on `st`.  The arguments have been validated; n_frames > 0.
// own_plan_ws: the caller's own block for the work list (a pipe's batch; ctx_plan_ws_bytes(n_frames) bytes, 256-byte
// aligned) — the launch then takes NOTHING from the context's scratch ring — and the pipe form of the launch: d_keep is
// one plane or null, no clear kernel, no info, flags and one count (the applied vector when report_vector) stored at
// system scope when `outputs_in_host_memory`.  nullptr: the ring, the stream form.
int gmc_on(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, uint64_t rebase, const uint64_t *d_off,
           const uint8_t *d_sd, uint32_t n_frames, int32_t max_shift, int32_t min_share_q8, uint8_t *d_flags, uint32_t *d_centres,
           mt_gmc_info *d_info, hipStream_t st, void *own_plan_ws = nullptr, const uint64_t *d_keep = nullptr,
           int report_vector = 0, int outputs_in_host_memory = 0) {
  mtgpu_gmc_plan gp;
  MT_TRY(gmc_plan(c->params, c->lds_max, &gp));
  mtgpu::GmcLaunch L;
  fill_batch(L, c, d_rec, rec_bytes, n_records, rebase, d_off, d_sd, n_frames, gp.lds_bytes, st);
  L.flags = d_flags; L.centres = d_centres; L.info = reinterpret_cast<unsigned int *>(d_info);
  fill_tile(L.k, c->k, mtgpu::gmc_tile_words);
  L.k.clust_need = c->k.clust_need;
  L.k.max_shift = (int)max_shift;
  L.k.min_share_q8 = (unsigned int)min_share_q8;
  if (own_plan_ws) {
    L.pipe = 1;
    L.keep = reinterpret_cast<const unsigned long long *>(d_keep);
    L.sys_flags = (d_flags && outputs_in_host_memory) ? 1 : 0;
    L.sys_centres = (d_centres && outputs_in_host_memory) ? 1 : 0;
    L.report_vector = report_vector ? 1 : 0;
  }
  PlanWs ws(c, st, own_plan_ws, mtgpu::ctx_plan_ws_bytes(n_frames));
  if (ws.rc != MT_OK) return ws.rc;
  L.plan_ws = ws.p;
  return profiled_launch(c, st, L, mtgpu::launch_gmc_scan, "compensated scan launch");
}

}  // namespace

namespace mtgpu {
int ctx_gmc_supported(const mtgpu_ctx *c) { return plan_ok(c, gmc_plan); }
int ctx_launch_gmc(mtgpu_ctx *c, const void *d_rec, uint64_t n_records, const uint64_t *d_off, const uint8_t *d_sd,
                   uint32_t n_frames, const uint64_t *d_keep, int32_t max_shift, int32_t min_share_q8, int report_vector,
                   uint8_t *d_flags, uint32_t *d_count, hipStream_t st, int rec_bytes, int outputs_in_host_memory, void *plan_ws,
                   size_t plan_ws_bytes) {
  if (n_frames == 0) return MT_OK;
  MT_TRY(gmc_check_settings(max_shift, min_share_q8));
  if (report_vector && !d_count) return fail(MT_ERR_INVALID, "compensated pipe scan: the vector report needs the batch's count array");
  MT_TRY(check_pipe_ws("compensated", plan_ws, plan_ws_bytes, n_frames));
  return gmc_on(c, d_rec, rec_bytes, n_records, 0, d_off, d_sd, n_frames, max_shift, min_share_q8, d_flags, d_count, nullptr, st,
                plan_ws, d_keep, report_vector ? 1 : 0, outputs_in_host_memory ? 1 : 0);
}
}  // namespace mtgpu

extern "C" {

int mtgpu_gmc_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, mtgpu_gmc_plan *out) {
  return preview(p, lds_bytes_per_workgroup, out, gmc_plan);
}

int mtgpu_scan_gmc_device(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, const uint64_t *d_frame_off,
                          const uint8_t *d_has_sd, uint32_t n_frames, int32_t max_shift, int32_t min_share_q8, uint8_t *d_flags,
                          uint32_t *d_centres, mt_gmc_info *d_info, void *stream) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(check_rec_bytes(rec_bytes));
  MT_TRY(gmc_check_settings(max_shift, min_share_q8));
  MT_TRY(check_any_output("d_", {{"flags", d_flags}, {"centres", d_centres}, {"info", d_info}}));
  if (n_frames > 0 && !d_frame_off) return fail(MT_ERR_INVALID, "d_frame_off is NULL");
  MT_TRY(check_aligned("d_", {{"frame_off", d_frame_off, 8}}));
  if (n_frames > 0 && n_records > 0 && !d_rec) return fail(MT_ERR_INVALID, "d_rec is NULL with n_records > 0");
  MT_TRY(check_rec("d_", rec_bytes, d_rec));
  MT_TRY(check_aligned("d_", {{"centres", d_centres, 4}, {"info", d_info, 4}}));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(plan_ok(c, gmc_plan));                              // a grid without a form: before any HIP call
  if (n_frames == 0) return MT_OK;
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_on_device(c, {{"d_flags", d_flags}, {"d_centres", d_centres}, {"d_info", d_info}}));
  MT_TRY(check_offsets_on(c, d_frame_off, n_frames, stream));
  return gmc_on(c, d_rec, rec_bytes, n_records, 0, d_frame_off, d_has_sd, n_frames, max_shift, min_share_q8, d_flags, d_centres,
                d_info, static_cast<hipStream_t>(stream));
}

int mtgpu_scan_frames_gmc(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd, uint32_t n_frames,
                          int32_t max_shift, int32_t min_share_q8, uint8_t *flags, uint32_t *centres, mt_gmc_info *info) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(gmc_check_settings(max_shift, min_share_q8));
  MT_TRY(check_any_output("", {{"flags", flags}, {"centres", centres}, {"info", info}}));
  if (n_frames > 0 && !frame_off) return fail(MT_ERR_INVALID, "frame_off is NULL");
  MT_TRY(check_monotonic("frame_off", "frame", frame_off, n_frames));
  uint64_t r_begin, r_end;
  MT_TRY(check_window(mv, frame_off, n_frames, &r_begin, &r_end));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(plan_ok(c, gmc_plan));                              // a grid without a form: before anything is staged
  if (n_frames == 0) return MT_OK;

  Staged sg(c, c->d_misc, false, mv, r_begin, r_end, frame_off, has_sd, n_frames);
  const int o_fl = sg.out(flags, n_frames), o_cen = sg.out(centres, sizeof(uint32_t) * (size_t)n_frames);
  const int o_info = sg.out(info, sizeof(mt_gmc_info) * (size_t)n_frames);
  MT_TRY(sg.upload());
  MT_TRY(gmc_on(c, sg.d_mv(), MT_MV_BYTES, r_end, r_begin, sg.d_off(), sg.d_sd(), n_frames, max_shift, min_share_q8, sg.at<uint8_t>(o_fl),
                sg.at<uint32_t>(o_cen), sg.at<mt_gmc_info>(o_info), sg.st));
  return sg.download();
}

}  // extern "C"

// ---------------------------------------------------------------- the compensated blob scan (src/motion_scanner.cpp:246-294
// per frame on the residuals of the frame's dominant vector, then the components of the centres; include/mtgpu_gmc_blobs.h)

namespace {

static_assert(MT_PIPE_REPORT_CENTRES == mtgpu::kGmcBlobReportCentres && MT_PIPE_REPORT_LARGEST == mtgpu::kGmcBlobReportLargest &&
              MT_PIPE_REPORT_VECTOR == mtgpu::kGmcBlobReportVector, "the kernel's report values are the ABI's");

// One form: the blob scan's layout and the two histograms.  It fits or the grid is unsupported.
int gmc_blobs_plan(const mt_scan_params &p, int lds_max, mtgpu_gmc_blobs_plan *out) {
  const int R = analysed_rows(p);
  const long long need = (long long)mtgpu::gmc_blobs_lds_bytes(p.grid_w, R);
  if (need > (long long)lds_max)
    return fail(MT_ERR_UNSUPPORTED, "grid %dx%d: one tile of 32-bit counters for %d rows, the keep rows, one mask plane and the "
                "histograms (%lld bytes) do not fit %d bytes of LDS; the compensated blob scan has no banded form", p.grid_w,
                p.grid_h, R + 2, need, lds_max);
  const long long W = ((long long)p.grid_w + 63) / 64;
  out->lds_bytes = (int32_t)need;
  out->workgroup = mtgpu::kGmcBlobBlock;
  out->keep_words_per_row = (int32_t)W;
  out->keep_words_per_stream = (int32_t)(W * (long long)p.grid_h);
  out->hist_bins = mtgpu::kGmcHistBins;
  out->info_bytes = (int32_t)sizeof(mt_gmc_info);
  return MT_OK;
}

// The compensated blob scan of a device-resident batch on `st`.  The arguments have been validated; n_frames > 0.
// own_plan_ws (include/mtgpu_pipe_gmc_blobs.h): the caller's own block for the work list (a pipe's batch) — nothing
// comes from the context's scratch ring — and the pipe form of the launch: d_keep is one plane or null and there is no
// stream table, d_centres is the batch's ONE count array and receives what `report` says, d_blobs, d_largest and d_info
// are null, flags and the count are stored at system scope when `outputs_in_host_memory`.  nullptr: the ring, the
// resident form.
int gmc_blobs_on(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, uint64_t rebase, const uint64_t *d_off,
                 const uint8_t *d_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams, const uint64_t *d_keep,
                 int32_t max_shift, int32_t min_share_q8, int32_t min_blob_cells, uint8_t *d_flags, uint32_t *d_centres,
                 uint32_t *d_blobs, uint32_t *d_largest, mt_blob_box *d_box, mt_gmc_info *d_info, hipStream_t st,
                 void *own_plan_ws = nullptr, int report = 0, int outputs_in_host_memory = 0) {
  mtgpu_gmc_blobs_plan gp;
  MT_TRY(gmc_blobs_plan(c->params, c->lds_max, &gp));
  mtgpu::GmcBlobLaunch L;
  fill_batch(L, c, d_rec, rec_bytes, n_records, rebase, d_off, d_sd, n_frames, gp.lds_bytes, st);
  L.stream_off = reinterpret_cast<const unsigned long long *>(d_stream_off);
  L.n_streams = n_streams;
  L.keep = reinterpret_cast<const unsigned long long *>(d_keep);
  L.flags = d_flags; L.centres = d_centres; L.blobs = d_blobs; L.largest = d_largest;
  L.box = reinterpret_cast<mtgpu::BlobBox *>(d_box);          // (pipe form: nullptr is the form without boxes)
  L.info = reinterpret_cast<unsigned int *>(d_info);
  fill_tile(L.k, c->k, mtgpu::blob_tile_words);
  L.k.clust_need = c->k.clust_need;
  L.k.blob_need = min_blob_cells < 1 ? 1u : (unsigned int)min_blob_cells;
  L.k.max_shift = (int)max_shift;
  L.k.min_share_q8 = (unsigned int)min_share_q8;
  if (own_plan_ws) {
    L.pipe = 1;
    L.sys_flags = (d_flags && outputs_in_host_memory) ? 1 : 0;
    L.sys_count = (d_centres && outputs_in_host_memory) ? 1 : 0;
    L.report = report;
  }
  PlanWs ws(c, st, own_plan_ws, mtgpu::ctx_plan_ws_bytes(n_frames));
  if (ws.rc != MT_OK) return ws.rc;
  L.plan_ws = ws.p;
  return profiled_launch(c, st, L, mtgpu::launch_gmc_blob_scan,
                         own_plan_ws ? "compensated blob pipe scan launch" : "compensated blob scan launch");
}

}  // namespace

namespace mtgpu {
int ctx_launch_gmc_blobs(mtgpu_ctx *c, const void *d_rec, uint64_t n_records, const uint64_t *d_off, const uint8_t *d_sd,
                         uint32_t n_frames, const uint64_t *d_keep, int32_t max_shift, int32_t min_share_q8, int32_t min_blob_cells,
                         int report, uint8_t *d_flags, uint32_t *d_count, hipStream_t st, int rec_bytes, int outputs_in_host_memory,
                         void *plan_ws, size_t plan_ws_bytes, mt_blob_box *d_box) {
  if (n_frames == 0) return MT_OK;
  // (8-byte aligned as in ctx_launch_blobs, but asked first here)
  if (((uintptr_t)d_box & 7u) != 0u)
    return fail(MT_ERR_INVALID, "compensated blob pipe scan: the batch's box array must be 8-byte aligned");
  MT_TRY(gmc_check_settings(max_shift, min_share_q8));
  if (min_blob_cells < 1) return fail(MT_ERR_INVALID, "compensated blob pipe scan: min_blob_cells is %d, want >= 1", (int)min_blob_cells);
  if (report != MT_PIPE_REPORT_CENTRES && report != MT_PIPE_REPORT_LARGEST && report != MT_PIPE_REPORT_VECTOR)
    return fail(MT_ERR_INVALID, "compensated blob pipe scan: report is %d", report);
  if (report != MT_PIPE_REPORT_CENTRES && !d_count)
    return fail(MT_ERR_INVALID, "compensated blob pipe scan: the largest and the vector report need the batch's count array");
  MT_TRY(check_pipe_ws("compensated blob", plan_ws, plan_ws_bytes, n_frames));
  return gmc_blobs_on(c, d_rec, rec_bytes, n_records, 0, d_off, d_sd, n_frames, nullptr, 0, d_keep, max_shift, min_share_q8,
                      min_blob_cells, d_flags, d_count, nullptr, nullptr, d_box, nullptr, st, plan_ws, report,
                      outputs_in_host_memory ? 1 : 0);
}
int ctx_gmc_blobs_supported(const mtgpu_ctx *c) { return plan_ok(c, gmc_blobs_plan); }
}  // namespace mtgpu

extern "C" {

int mtgpu_gmc_blobs_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, mtgpu_gmc_blobs_plan *out) {
  return preview(p, lds_bytes_per_workgroup, out, gmc_blobs_plan);
}

int mtgpu_scan_gmc_blobs_device(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, const uint64_t *d_frame_off,
                                const uint8_t *d_has_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams,
                                const uint64_t *d_keep, int32_t max_shift, int32_t min_share_q8, int32_t min_blob_cells,
                                uint8_t *d_flags, uint32_t *d_centres, uint32_t *d_blobs, uint32_t *d_largest, mt_blob_box *d_box,
                                mt_gmc_info *d_info, void *stream) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(check_rec_bytes(rec_bytes));
  MT_TRY(gmc_check_settings(max_shift, min_share_q8));
  MT_TRY(check_any_output("d_", {{"flags", d_flags}, {"centres", d_centres}, {"blobs", d_blobs}, {"largest", d_largest}, {"box", d_box},
                                 {"info", d_info}}));
  if (n_frames > 0 && !d_frame_off) return fail(MT_ERR_INVALID, "d_frame_off is NULL");
  MT_TRY(check_stream_table("d_", d_stream_off, n_streams, d_keep));
  MT_TRY(check_aligned("d_", {{"frame_off", d_frame_off, 8}, {"stream_off", d_stream_off, 8}, {"keep", d_keep, 8}}));
  if (n_frames > 0 && n_records > 0 && !d_rec) return fail(MT_ERR_INVALID, "d_rec is NULL with n_records > 0");
  MT_TRY(check_rec("d_", rec_bytes, d_rec));
  MT_TRY(check_aligned("d_", {{"centres", d_centres, 4}, {"blobs", d_blobs, 4}, {"largest", d_largest, 4}, {"box", d_box, 2},
                              {"info", d_info, 4}}));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(plan_ok(c, gmc_blobs_plan));                        // a grid without a form: before any HIP call
  if (n_frames == 0) return MT_OK;
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_on_device(c, {{"d_keep", d_keep}, {"d_flags", d_flags}, {"d_centres", d_centres}, {"d_blobs", d_blobs},
                             {"d_largest", d_largest}, {"d_box", d_box}, {"d_info", d_info}}));
  MT_TRY(check_offsets_on(c, d_frame_off, n_frames, stream));
  return gmc_blobs_on(c, d_rec, rec_bytes, n_records, 0, d_frame_off, d_has_sd, n_frames, d_stream_off, n_streams, d_keep,
                      max_shift, min_share_q8, min_blob_cells, d_flags, d_centres, d_blobs, d_largest, d_box, d_info,
                      static_cast<hipStream_t>(stream));
}

int mtgpu_scan_frames_gmc_blobs(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd, uint32_t n_frames,
                                const uint64_t *stream_off, uint32_t n_streams, const uint64_t *keep, int32_t max_shift,
                                int32_t min_share_q8, int32_t min_blob_cells, uint8_t *flags, uint32_t *centres, uint32_t *blobs,
                                uint32_t *largest, mt_blob_box *box, mt_gmc_info *info) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(gmc_check_settings(max_shift, min_share_q8));
  MT_TRY(check_any_output("", {{"flags", flags}, {"centres", centres}, {"blobs", blobs}, {"largest", largest}, {"box", box}, {"info", info}}));
  if (n_frames > 0 && !frame_off) return fail(MT_ERR_INVALID, "frame_off is NULL");
  MT_TRY(check_stream_table("", stream_off, n_streams, keep));
  MT_TRY(check_monotonic("frame_off", "frame", frame_off, n_frames));
  if (keep) MT_TRY(check_stream_off(stream_off, n_streams, n_frames));
  uint64_t r_begin, r_end;
  MT_TRY(check_window(mv, frame_off, n_frames, &r_begin, &r_end));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(plan_ok(c, gmc_blobs_plan));                        // a grid without a form: before anything is staged
  if (n_frames == 0) return MT_OK;

  // (without a mask stream_off and keep are null and n_streams is 0: no room, null device pointers)
  const size_t words = sizeof(uint32_t) * (size_t)n_frames;
  Staged sg(c, c->d_misc, false, mv, r_begin, r_end, frame_off, has_sd, n_frames);
  const int i_soff = sg.in(stream_off, sizeof(uint64_t) * ((size_t)n_streams + 1));
  const int i_keep = sg.in(keep, sizeof(uint64_t) * (size_t)n_streams * (size_t)c->k.gh * (size_t)c->k.W);
  const int o_fl = sg.out(flags, n_frames), o_cen = sg.out(centres, words), o_bl = sg.out(blobs, words), o_lg = sg.out(largest, words);
  const int o_box = sg.out(box, sizeof(mt_blob_box) * (size_t)n_frames), o_info = sg.out(info, sizeof(mt_gmc_info) * (size_t)n_frames);
  MT_TRY(sg.upload());
  MT_TRY(gmc_blobs_on(c, sg.d_mv(), MT_MV_BYTES, r_end, r_begin, sg.d_off(), sg.d_sd(), n_frames, sg.at<const uint64_t>(i_soff),
                      n_streams, sg.at<const uint64_t>(i_keep), max_shift, min_share_q8, min_blob_cells, sg.at<uint8_t>(o_fl),
                      sg.at<uint32_t>(o_cen), sg.at<uint32_t>(o_bl), sg.at<uint32_t>(o_lg), sg.at<mt_blob_box>(o_box),
                      sg.at<mt_gmc_info>(o_info), sg.st));
  return sg.download();
}

}  // extern "C"


// ---------------------------------------------------------------- temporal persistence (include/mtgpu_persist.h)

namespace {

static_assert(sizeof(mtgpu::PersistBox) == sizeof(mt_blob_box), "the kernel's box is the ABI's");

struct PersistRange { const char *name; const void *p; size_t bytes; };

// What the arguments of a persistence call decide alone (`d`: "d_" for the device entry point, "" for the host one):
// no context, no device.
int persist_check_args(const char *d, const void *flags, const void *has_sd, const void *box, uint32_t n_frames,
                       const void *stream_off, uint32_t n_streams, uint32_t reach, const void *work, bool need_work,
                       const void *flags_out, const void *run, const void *pos) {
  if (!flags_out && !run && !pos) return fail(MT_ERR_INVALID, "%sflags_out, %srun and %spos are all NULL", d, d, d);
  if (reach > 65535u) return fail(MT_ERR_INVALID, "reach %u outside [0,65535]", reach);
  if (n_frames > 0 && !flags) return fail(MT_ERR_INVALID, "%sflags is NULL", d);
  if (n_frames > 0 && !stream_off) return fail(MT_ERR_INVALID, "%sstream_off is NULL", d);
  if (n_frames > 0 && need_work && !work) return fail(MT_ERR_INVALID, "%swork is NULL", d);
  if (n_frames > 0 && n_streams == 0) return fail(MT_ERR_INVALID, "n_streams is 0 with n_frames %u", n_frames);
  if (((uintptr_t)stream_off & 7u) != 0) return fail(MT_ERR_INVALID, "%sstream_off must be 8-byte aligned", d);
  if (((uintptr_t)box & 1u) != 0) return fail(MT_ERR_INVALID, "%sbox must be 2-byte aligned", d);
  if (((uintptr_t)work & 3u) != 0) return fail(MT_ERR_INVALID, "%swork must be 4-byte aligned", d);
  if (((uintptr_t)run & 3u) != 0) return fail(MT_ERR_INVALID, "%srun must be 4-byte aligned", d);
  if (((uintptr_t)pos & 3u) != 0) return fail(MT_ERR_INVALID, "%spos must be 4-byte aligned", d);
  // no in-place form: an output or the workspace shares no byte with an input or with another of them
  const size_t n = n_frames;
  const PersistRange r[8] = {{"flags", flags, n}, {"has_sd", has_sd, n}, {"box", box, n * sizeof(mt_blob_box)},
                             {"stream_off", stream_off, ((size_t)n_streams + 1) * sizeof(uint64_t)},
                             {"work", work, n * sizeof(uint32_t)}, {"flags_out", flags_out, n},
                             {"run", run, n * sizeof(uint32_t)}, {"pos", pos, n * sizeof(uint32_t)}};
  for (int i = 4; i < 8 && n > 0; ++i) {                      // r[4 ..]: the workspace and the outputs
    if (!r[i].p) continue;
    for (int j = 0; j < i; ++j) {
      if (!r[j].p) continue;
      const uintptr_t a0 = (uintptr_t)r[i].p, a1 = a0 + r[i].bytes, b0 = (uintptr_t)r[j].p, b1 = b0 + r[j].bytes;
      if (a0 < b1 && b0 < a1) return fail(MT_ERR_INVALID, "%s%s overlaps %s%s: there is no in-place form", d, r[i].name, d, r[j].name);
    }
  }
  return MT_OK;
}

int persist_on(const uint8_t *d_flags, const uint8_t *d_sd, const mt_blob_box *d_box, uint32_t n_frames, const uint64_t *d_stream_off,
               uint32_t n_streams, uint32_t min_run, uint32_t max_dropout, uint32_t reach, uint32_t *d_work, uint8_t *d_flags_out,
               uint32_t *d_run, uint32_t *d_pos, hipStream_t st) {
  mtgpu::PersistLaunch L;
  L.flags = d_flags;
  L.has_sd = d_sd;
  L.box = reinterpret_cast<const mtgpu::PersistBox *>(d_box);
  L.n_frames = n_frames;
  L.stream_off = reinterpret_cast<const unsigned long long *>(d_stream_off);
  L.n_streams = n_streams;
  L.need = min_run < 1u ? 1u : min_run;
  L.max_dropout = max_dropout;
  L.reach = d_box ? reach : 0u;
  L.work = d_work;
  L.flags_out = d_flags_out;
  L.run = d_run;
  L.pos = d_pos;
  L.stream = st;
  const hipError_t e = mtgpu::launch_persist(L);
  if (e != hipSuccess) return hip_fail(e, "persistence launch");
  return MT_OK;
}

}  // namespace

extern "C" {

int mtgpu_persist_preview(mtgpu_persist_plan *out) {
  if (!out) return fail(MT_ERR_INVALID, "out is NULL");
  out->workgroup = mtgpu::kPersistBlock;
  out->frames_per_tile = mtgpu::kPersistTile;
  return MT_OK;
}

int mtgpu_persist_flags_device(mtgpu_ctx *c, const uint8_t *d_flags, const uint8_t *d_has_sd, const mt_blob_box *d_box, uint32_t n_frames,
                               const uint64_t *d_stream_off, uint32_t n_streams, uint32_t min_run, uint32_t max_dropout, uint32_t reach,
                               uint32_t *d_work, uint8_t *d_flags_out, uint32_t *d_run, uint32_t *d_pos, void *stream) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  int rc = persist_check_args("d_", d_flags, d_has_sd, d_box, n_frames, d_stream_off, n_streams, reach, d_work, true, d_flags_out,
                              d_run, d_pos);
  if (rc != MT_OK) return rc;
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (n_frames == 0) return MT_OK;
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_on_device(c, {{"d_work", d_work}, {"d_flags_out", d_flags_out}, {"d_run", d_run}, {"d_pos", d_pos}}));
  return persist_on(d_flags, d_has_sd, d_box, n_frames, d_stream_off, n_streams, min_run, max_dropout, reach, d_work, d_flags_out,
                    d_run, d_pos, static_cast<hipStream_t>(stream));
}

int mtgpu_persist_flags(mtgpu_ctx *c, const uint8_t *flags, const uint8_t *has_sd, const mt_blob_box *box, uint32_t n_frames,
                        const uint64_t *stream_off, uint32_t n_streams, uint32_t min_run, uint32_t max_dropout, uint32_t reach,
                        uint8_t *flags_out, uint32_t *run, uint32_t *pos) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  int rc = persist_check_args("", flags, has_sd, box, n_frames, stream_off, n_streams, reach, nullptr, false, flags_out, run, pos);
  if (rc != MT_OK) return rc;
  if (n_frames > 0) {
    for (uint32_t s = 0; s < n_streams; ++s)
      if (stream_off[s + 1] < stream_off[s]) return fail(MT_ERR_INVALID, "stream_off not monotonic at stream %u", s);
    if (stream_off[n_streams] > (uint64_t)n_frames)
      return fail(MT_ERR_INVALID, "stream_off[%u] is %llu, above n_frames %u", n_streams, (unsigned long long)stream_off[n_streams], n_frames);
  }
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (n_frames == 0) return MT_OK;

  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = n_frames, words = sizeof(uint32_t) * n, soff_bytes = sizeof(uint64_t) * ((size_t)n_streams + 1);
  const auto up = [](size_t v) { return (v + 255u) & ~(size_t)255u; };
  const size_t o_soff = 0, o_fl = o_soff + up(soff_bytes), o_sd = o_fl + up(n), o_box = o_sd + (has_sd ? up(n) : 0),
               o_work = o_box + (box ? up(sizeof(mt_blob_box) * n) : 0), o_out = o_work + up(words), o_run = o_out + (flags_out ? up(n) : 0),
               o_pos = o_run + (run ? up(words) : 0), total = o_pos + (pos ? up(words) : 0);
  if ((rc = c->d_misc.reserve(total)) != MT_OK) return rc;
  unsigned char *d = static_cast<unsigned char *>(c->d_misc.p);
  hipStream_t st = c->stream;
  DrainOnExit drain{st};
  HIP_TRY(hipMemcpyAsync(d + o_soff, stream_off, soff_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d + o_fl, flags, n, hipMemcpyHostToDevice, st));
  if (has_sd) HIP_TRY(hipMemcpyAsync(d + o_sd, has_sd, n, hipMemcpyHostToDevice, st));
  if (box) HIP_TRY(hipMemcpyAsync(d + o_box, box, sizeof(mt_blob_box) * n, hipMemcpyHostToDevice, st));
  rc = persist_on(d + o_fl, has_sd ? d + o_sd : nullptr, box ? reinterpret_cast<const mt_blob_box *>(d + o_box) : nullptr, n_frames,
                  reinterpret_cast<const uint64_t *>(d + o_soff), n_streams, min_run, max_dropout, reach,
                  reinterpret_cast<uint32_t *>(d + o_work), flags_out ? d + o_out : nullptr,
                  run ? reinterpret_cast<uint32_t *>(d + o_run) : nullptr, pos ? reinterpret_cast<uint32_t *>(d + o_pos) : nullptr, st);
  if (rc != MT_OK) return rc;
  if (flags_out) HIP_TRY(hipMemcpyAsync(flags_out, d + o_out, n, hipMemcpyDeviceToHost, st));
  if (run) HIP_TRY(hipMemcpyAsync(run, d + o_run, words, hipMemcpyDeviceToHost, st));
  if (pos) HIP_TRY(hipMemcpyAsync(pos, d + o_pos, words, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return MT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- object tracks (include/mtgpu_tracks.h)

namespace {

static_assert(sizeof(mtgpu::TrackObject) == sizeof(mt_object) && sizeof(mt_object) == 16, "the kernel's list entry is the ABI's");
static_assert(mtgpu::kTracksGroup == MT_OBJECTS_MAX, "one lane per list entry");

struct TracksRange { const char *name; const void *p; size_t bytes; };

// What the arguments of a tracks call decide alone (`d`: "d_" for the device entry point, "" for the host one): no
// context, no device.  The rungs are persistence's, with k and the size limit in front of what they size.
int tracks_check_args(const char *d, const void *flags, const void *has_sd, const void *list, int32_t k, uint32_t n_frames,
                      const void *stream_off, uint32_t n_streams, uint32_t reach, const void *work, bool device, const void *pred,
                      const void *age, const void *id, const void *len, const void *track, const void *flags_out) {
  MT_TRY(check_any_output(d, {{"pred", pred}, {"age", age}, {"id", id}, {"len", len}, {"track", track}, {"flags_out", flags_out}}));
  if (k < 1 || k > MT_OBJECTS_MAX) return fail(MT_ERR_INVALID, "k is %d, outside [1,%d]", k, MT_OBJECTS_MAX);
  if ((uint64_t)n_frames * (uint64_t)k >= 0xFFFFFFFFull)
    return fail(MT_ERR_INVALID, "n_frames %u x k %d is not below 4294967295", n_frames, k);
  if (reach > 65535u) return fail(MT_ERR_INVALID, "reach %u outside [0,65535]", reach);
  if (n_frames > 0 && !flags) return fail(MT_ERR_INVALID, "%sflags is NULL", d);
  if (n_frames > 0 && !list) return fail(MT_ERR_INVALID, "%slist is NULL", d);
  if (n_frames > 0 && !stream_off) return fail(MT_ERR_INVALID, "%sstream_off is NULL", d);
  if (n_frames > 0 && device && !work) return fail(MT_ERR_INVALID, "%swork is NULL", d);
  if (n_frames > 0 && n_streams == 0) return fail(MT_ERR_INVALID, "n_streams is 0 with n_frames %u", n_frames);
  MT_TRY(check_aligned(d, {{"stream_off", stream_off, 8}, {"list", device ? list : nullptr, 16}, {"work", work, 4}, {"age", age, 4},
                           {"id", id, 4}, {"len", len, 4}, {"track", track, 4}}));
  // no in-place form: an output or the workspace shares no byte with an input or with another of them
  const size_t n = n_frames, nk = n * (size_t)k;
  const TracksRange r[11] = {{"flags", flags, n}, {"has_sd", has_sd, n}, {"list", list, nk * sizeof(mt_object)},
                             {"stream_off", stream_off, ((size_t)n_streams + 1) * sizeof(uint64_t)},
                             {"work", work, nk * sizeof(uint32_t) * mtgpu::kTracksWorkWords}, {"pred", pred, nk},
                             {"age", age, nk * sizeof(uint32_t)}, {"id", id, nk * sizeof(uint32_t)}, {"len", len, nk * sizeof(uint32_t)},
                             {"track", track, n * sizeof(uint32_t)}, {"flags_out", flags_out, n}};
  for (int i = 4; i < 11 && n > 0; ++i) {                     // r[4 ..]: the workspace and the outputs
    if (!r[i].p) continue;
    for (int j = 0; j < i; ++j) {
      if (!r[j].p) continue;
      const uintptr_t a0 = (uintptr_t)r[i].p, a1 = a0 + r[i].bytes, b0 = (uintptr_t)r[j].p, b1 = b0 + r[j].bytes;
      if (a0 < b1 && b0 < a1) return fail(MT_ERR_INVALID, "%s%s overlaps %s%s: there is no in-place form", d, r[i].name, d, r[j].name);
    }
  }
  return MT_OK;
}

int tracks_on(const uint8_t *d_flags, const uint8_t *d_sd, const mt_object *d_list, int32_t k, uint32_t n_frames, const uint64_t *d_stream_off,
              uint32_t n_streams, uint32_t min_cells, uint32_t max_dropout, uint32_t reach, uint32_t min_track, uint32_t *d_work,
              uint8_t *d_pred, uint32_t *d_age, uint32_t *d_id, uint32_t *d_len, uint32_t *d_track, uint8_t *d_flags_out, hipStream_t st) {
  mtgpu::TracksLaunch L;
  L.flags = d_flags;
  L.has_sd = d_sd;
  L.list = reinterpret_cast<const mtgpu::TrackObject *>(d_list);
  L.k = (unsigned int)k;
  L.n_frames = n_frames;
  L.stream_off = reinterpret_cast<const unsigned long long *>(d_stream_off);
  L.n_streams = n_streams;
  L.need_cells = min_cells < 1u ? 1u : min_cells;
  L.max_dropout = max_dropout;
  L.reach = reach;
  L.need_track = min_track < 1u ? 1u : min_track;
  L.work = d_work;
  L.pred = d_pred;
  L.age = d_age;
  L.id = d_id;
  L.len = d_len;
  L.track = d_track;
  L.flags_out = d_flags_out;
  L.stream = st;
  const hipError_t e = mtgpu::launch_tracks(L);
  if (e != hipSuccess) return hip_fail(e, "tracks launch");
  return MT_OK;
}

}  // namespace

extern "C" {

int mtgpu_tracks_preview(int k, mtgpu_tracks_plan *out) {
  if (!out) return fail(MT_ERR_INVALID, "out is NULL");
  if (k < 1 || k > MT_OBJECTS_MAX) return fail(MT_ERR_INVALID, "k is %d, outside [1,%d]", k, MT_OBJECTS_MAX);
  out->workgroup = mtgpu::kTracksBlock;
  out->frames_per_tile = mtgpu::kTracksTile;
  out->work_words_per_entry = mtgpu::kTracksWorkWords;
  return MT_OK;
}

int mtgpu_track_objects_device(mtgpu_ctx *c, const uint8_t *d_flags, const uint8_t *d_has_sd, const mt_object *d_list, int32_t k,
                               uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams, uint32_t min_cells, uint32_t max_dropout,
                               uint32_t reach, uint32_t min_track, uint32_t *d_work, uint8_t *d_pred, uint32_t *d_age, uint32_t *d_id,
                               uint32_t *d_len, uint32_t *d_track, uint8_t *d_flags_out, void *stream) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(tracks_check_args("d_", d_flags, d_has_sd, d_list, k, n_frames, d_stream_off, n_streams, reach, d_work, true, d_pred, d_age, d_id,
                           d_len, d_track, d_flags_out));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (n_frames == 0) return MT_OK;
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_on_device(c, {{"d_work", d_work}, {"d_pred", d_pred}, {"d_age", d_age}, {"d_id", d_id}, {"d_len", d_len}, {"d_track", d_track},
                             {"d_flags_out", d_flags_out}}));
  return tracks_on(d_flags, d_has_sd, d_list, k, n_frames, d_stream_off, n_streams, min_cells, max_dropout, reach, min_track, d_work, d_pred,
                   d_age, d_id, d_len, d_track, d_flags_out, static_cast<hipStream_t>(stream));
}

int mtgpu_track_objects(mtgpu_ctx *c, const uint8_t *flags, const uint8_t *has_sd, const mt_object *list, int32_t k, uint32_t n_frames,
                        const uint64_t *stream_off, uint32_t n_streams, uint32_t min_cells, uint32_t max_dropout, uint32_t reach,
                        uint32_t min_track, uint8_t *pred, uint32_t *age, uint32_t *id, uint32_t *len, uint32_t *track, uint8_t *flags_out) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(tracks_check_args("", flags, has_sd, list, k, n_frames, stream_off, n_streams, reach, nullptr, false, pred, age, id, len, track,
                           flags_out));
  if (n_frames > 0) {
    MT_TRY(check_monotonic("stream_off", "stream", stream_off, n_streams));
    if (stream_off[n_streams] > (uint64_t)n_frames)
      return fail(MT_ERR_INVALID, "stream_off[%u] is %llu, above n_frames %u", n_streams, (unsigned long long)stream_off[n_streams], n_frames);
  }
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  if (n_frames == 0) return MT_OK;

  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  // one block of d_misc, laid out by api_common.h's stage_layout: four inputs, the workspace, six outputs
  const size_t n = n_frames, nk = n * (size_t)k, words = sizeof(uint32_t) * nk;
  constexpr int kSlots = 11;
  void *const host[kSlots] = {const_cast<uint64_t *>(stream_off), const_cast<uint8_t *>(flags), const_cast<uint8_t *>(has_sd),
                              const_cast<mt_object *>(list), nullptr, pred, age, id, len, track, flags_out};
  const mtgpu::StageSlot slot[kSlots] = {{sizeof(uint64_t) * ((size_t)n_streams + 1), true}, {n, true}, {n, has_sd != nullptr},
                                         {sizeof(mt_object) * nk, true}, {words * mtgpu::kTracksWorkWords, true}, {nk, pred != nullptr},
                                         {words, age != nullptr}, {words, id != nullptr}, {words, len != nullptr},
                                         {sizeof(uint32_t) * n, track != nullptr}, {n, flags_out != nullptr}};
  size_t off[kSlots];
  MT_TRY(c->d_misc.reserve(mtgpu::stage_layout(slot, kSlots, false, off)));
  unsigned char *const d = static_cast<unsigned char *>(c->d_misc.p);
  const auto at = [&](int i) -> unsigned char * { return off[i] == mtgpu::kNoSlot ? nullptr : d + off[i]; };
  hipStream_t st = c->stream;
  DrainOnExit drain{st};
  for (int i = 0; i < 4; ++i)
    if (at(i)) HIP_TRY(hipMemcpyAsync(at(i), host[i], slot[i].bytes, hipMemcpyHostToDevice, st));
  MT_TRY(tracks_on(at(1), at(2), reinterpret_cast<const mt_object *>(at(3)), k, n_frames, reinterpret_cast<const uint64_t *>(at(0)), n_streams,
                   min_cells, max_dropout, reach, min_track, reinterpret_cast<uint32_t *>(at(4)), at(5), reinterpret_cast<uint32_t *>(at(6)),
                   reinterpret_cast<uint32_t *>(at(7)), reinterpret_cast<uint32_t *>(at(8)), reinterpret_cast<uint32_t *>(at(9)), at(10), st));
  for (int i = 5; i < kSlots; ++i)
    if (at(i)) HIP_TRY(hipMemcpyAsync(host[i], at(i), slot[i].bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return MT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- the direction filter (src/motion_scanner.cpp:242-292 per
// frame, the vote only for records of an allowed sector, and the per-frame rose; include/mtgpu_dir.h)

namespace {

static_assert(sizeof(mt_dir_rose) == 32 && alignof(mt_dir_rose) == 4, "mt_dir_rose is eight uint32");

// One form: the tile, one mask plane, the total and the eight rose words.  It fits or the grid is unsupported.
int dir_plan(const mt_scan_params &p, int lds_max, mtgpu_dir_plan *out) {
  const int R = analysed_rows(p);
  const long long need = (long long)mtgpu::dir_lds_bytes(p.grid_w, R);
  if (need > (long long)lds_max)
    return fail(MT_ERR_UNSUPPORTED, "grid %dx%d: one tile of 32-bit counters for %d rows, one mask plane and the rose "
                "(%lld bytes) do not fit %d bytes of LDS; the direction scan has no banded form", p.grid_w, p.grid_h, R + 2, need, lds_max);
  out->lds_bytes = (int32_t)need;
  out->workgroup = mtgpu::kDirBlock;
  out->sectors = 8;
  out->rose_bytes = (int32_t)sizeof(mt_dir_rose);
  return MT_OK;
}

// What the arguments of a direction call decide alone (`d`: "d_" for the device entry point, "" for the host one): no
// context, no device.
int dir_check_args(const char *d, const char *allow_name, int rec_bytes, const void *rec, const void *frame_off, uint32_t n_frames,
                   const void *stream_off, uint32_t n_streams, const void *allows, int32_t allow, const void *flags,
                   const void *centres, const void *rose) {
  if (allow < 0 || allow > 255) return fail(MT_ERR_INVALID, "allow %d outside [0,255]", (int)allow);
  MT_TRY(check_rec_bytes(rec_bytes));
  MT_TRY(check_any_output(d, {{"flags", flags}, {"centres", centres}, {"rose", rose}}));
  if (n_frames > 0 && !frame_off) return fail(MT_ERR_INVALID, "%sframe_off is NULL", d);
  // check_stream_table's rule about the per-stream allow bytes, in this call's own words
  if (allows) {
    if (!stream_off) return fail(MT_ERR_INVALID, "%s%s is given and %sstream_off is NULL", d, allow_name, d);
    if (n_streams == 0) return fail(MT_ERR_INVALID, "%s%s is given and n_streams is 0", d, allow_name);
  } else {
    if (stream_off) return fail(MT_ERR_INVALID, "%sstream_off is given and %s%s is NULL", d, d, allow_name);
    if (n_streams != 0) return fail(MT_ERR_INVALID, "n_streams is %u and %s%s is NULL", n_streams, d, allow_name);
  }
  MT_TRY(check_aligned(d, {{"frame_off", frame_off, 8}, {"stream_off", stream_off, 8}}));
  MT_TRY(check_rec(d, rec_bytes, rec));
  return check_aligned(d, {{"centres", centres, 4}, {"rose", rose, 4}});
}

// The direction scan of a device-resident batch on `st`.  The arguments have been validated; n_frames > 0.
// own_plan_ws: the caller's own block for the work list (a pipe's batch; ctx_plan_ws_bytes(n_frames) bytes, 256-byte
// aligned) — the launch then takes NOTHING from the context's scratch ring — and the pipe form of the launch: d_keep is
// one plane or null, no clear kernel, no stream lookup, no rose, flags and one count (the sector word when
// report_sectors) stored at system scope when `outputs_in_host_memory`.  nullptr: the ring, the stream form.
int dir_on(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, uint64_t rebase, const uint64_t *d_off,
           const uint8_t *d_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams, const uint8_t *d_allow,
           int32_t allow, uint8_t *d_flags, uint32_t *d_centres, mt_dir_rose *d_rose, hipStream_t st, void *own_plan_ws = nullptr,
           const uint64_t *d_keep = nullptr, int report_sectors = 0, int outputs_in_host_memory = 0) {
  mtgpu_dir_plan dp;
  MT_TRY(dir_plan(c->params, c->lds_max, &dp));
  mtgpu::DirLaunch L;
  fill_batch(L, c, d_rec, rec_bytes, n_records, rebase, d_off, d_sd, n_frames, dp.lds_bytes, st);
  L.stream_off = reinterpret_cast<const unsigned long long *>(d_stream_off);
  L.n_streams = n_streams;
  L.allows = d_allow;
  L.allow = (unsigned int)allow;
  L.flags = d_flags; L.centres = d_centres; L.rose = reinterpret_cast<unsigned int *>(d_rose);
  fill_tile(L.k, c->k, mtgpu::dir_tile_words);
  L.k.clust_need = c->k.clust_need;
  if (own_plan_ws) {
    L.pipe = 1;
    L.keep = reinterpret_cast<const unsigned long long *>(d_keep);
    L.sys_flags = (d_flags && outputs_in_host_memory) ? 1 : 0;
    L.sys_centres = (d_centres && outputs_in_host_memory) ? 1 : 0;
    L.report_sectors = report_sectors ? 1 : 0;
  }
  PlanWs ws(c, st, own_plan_ws, mtgpu::ctx_plan_ws_bytes(n_frames));
  if (ws.rc != MT_OK) return ws.rc;
  L.plan_ws = ws.p;
  return profiled_launch(c, st, L, mtgpu::launch_dir_scan, "direction scan launch");
}

}  // namespace

namespace mtgpu {
int ctx_dir_supported(const mtgpu_ctx *c) { return plan_ok(c, dir_plan); }
int ctx_launch_dir(mtgpu_ctx *c, const void *d_rec, uint64_t n_records, const uint64_t *d_off, const uint8_t *d_sd,
                   uint32_t n_frames, const uint64_t *d_keep, int32_t allow, int report_sectors, uint8_t *d_flags,
                   uint32_t *d_count, hipStream_t st, int rec_bytes, int outputs_in_host_memory, void *plan_ws,
                   size_t plan_ws_bytes) {
  if (n_frames == 0) return MT_OK;
  if (allow < 0 || allow > 255) return fail(MT_ERR_INVALID, "allow %d outside [0,255]", (int)allow);
  if (report_sectors && !d_count) return fail(MT_ERR_INVALID, "direction pipe scan: the sector report needs the batch's count array");
  MT_TRY(check_pipe_ws("direction", plan_ws, plan_ws_bytes, n_frames));
  return dir_on(c, d_rec, rec_bytes, n_records, 0, d_off, d_sd, n_frames, nullptr, 0, nullptr, allow, d_flags, d_count, nullptr, st,
                plan_ws, d_keep, report_sectors ? 1 : 0, outputs_in_host_memory ? 1 : 0);
}
}  // namespace mtgpu

extern "C" {

int mtgpu_dir_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, mtgpu_dir_plan *out) {
  return preview(p, lds_bytes_per_workgroup, out, dir_plan);
}

int mtgpu_scan_dir_device(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, const uint64_t *d_frame_off,
                          const uint8_t *d_has_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams,
                          const uint8_t *d_allow, int32_t allow, uint8_t *d_flags, uint32_t *d_centres, mt_dir_rose *d_rose,
                          void *stream) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(dir_check_args("d_", "allow", rec_bytes, d_rec, d_frame_off, n_frames, d_stream_off, n_streams, d_allow, allow, d_flags,
                        d_centres, d_rose));
  // (behind the alignment rungs here; the other device forms ask before them)
  if (n_frames > 0 && n_records > 0 && !d_rec) return fail(MT_ERR_INVALID, "d_rec is NULL with n_records > 0");
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(plan_ok(c, dir_plan));                              // a grid without a form: before any HIP call
  if (n_frames == 0) return MT_OK;
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_on_device(c, {{"d_flags", d_flags}, {"d_centres", d_centres}, {"d_rose", d_rose}}));
  MT_TRY(check_offsets_on(c, d_frame_off, n_frames, stream));
  return dir_on(c, d_rec, rec_bytes, n_records, 0, d_frame_off, d_has_sd, n_frames, d_stream_off, n_streams, d_allow, allow, d_flags,
                d_centres, d_rose, static_cast<hipStream_t>(stream));
}

int mtgpu_scan_frames_dir(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd, uint32_t n_frames,
                          const uint64_t *stream_off, uint32_t n_streams, const uint8_t *allows, int32_t allow, uint8_t *flags,
                          uint32_t *centres, mt_dir_rose *rose) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  // (the one host form with alignment rungs: it shares its checker with the device form)
  MT_TRY(dir_check_args("", "allows", MT_MV_BYTES, mv, frame_off, n_frames, stream_off, n_streams, allows, allow, flags, centres, rose));
  MT_TRY(check_monotonic("frame_off", "frame", frame_off, n_frames));
  if (allows) MT_TRY(check_stream_off(stream_off, n_streams, n_frames));
  uint64_t r_begin, r_end;
  MT_TRY(check_window(mv, frame_off, n_frames, &r_begin, &r_end));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(plan_ok(c, dir_plan));                              // a grid without a form: before anything is staged
  if (n_frames == 0) return MT_OK;

  // (without per-stream bytes stream_off and allows are null: no room, null device pointers)
  Staged sg(c, c->d_misc, false, mv, r_begin, r_end, frame_off, has_sd, n_frames);
  const int i_soff = sg.in(stream_off, sizeof(uint64_t) * ((size_t)n_streams + 1)), i_allow = sg.in(allows, n_streams);
  const int o_fl = sg.out(flags, n_frames), o_cen = sg.out(centres, sizeof(uint32_t) * (size_t)n_frames);
  const int o_rose = sg.out(rose, sizeof(mt_dir_rose) * (size_t)n_frames);
  MT_TRY(sg.upload());
  MT_TRY(dir_on(c, sg.d_mv(), MT_MV_BYTES, r_end, r_begin, sg.d_off(), sg.d_sd(), n_frames, sg.at<const uint64_t>(i_soff), n_streams,
                sg.at<const uint8_t>(i_allow), allow, sg.at<uint8_t>(o_fl), sg.at<uint32_t>(o_cen), sg.at<mt_dir_rose>(o_rose), sg.st));
  return sg.download();
}

}  // extern "C"

// ---------------------------------------------------------------- direction planes (src/motion_scanner.cpp:242-292 per
// frame, the vote only for records whose sector the destination cell's byte allows; the flow map: the counting records
// per stream, sector and cell; include/mtgpu_lanes.h)

namespace {

// Two forms: the direction scan's LDS with the plane's analysed rows behind it, or without them.  The direction scan's
// part fits or the grid is unsupported.
int lanes_plan(const mt_scan_params &p, int lds_max, mtgpu_lanes_plan *out) {
  const int R = analysed_rows(p);
  const long long base = (long long)mtgpu::lanes_lds_bytes(p.grid_w, R, false);
  const long long with_rows = (long long)mtgpu::lanes_lds_bytes(p.grid_w, R, true);
  if (base > (long long)lds_max)
    return fail(MT_ERR_UNSUPPORTED, "grid %dx%d: one tile of 32-bit counters for %d rows, one mask plane and the rose "
                "(%lld bytes) do not fit %d bytes of LDS; the plane scan has no banded form", p.grid_w, p.grid_h, R + 2, base, lds_max);
  out->staged = with_rows <= (long long)lds_max ? 1 : 0;
  out->lds_bytes = (int32_t)(out->staged ? with_rows : base);
  out->workgroup = mtgpu::kLanesBlock;
  out->plane_bytes = (int32_t)((long long)p.grid_w * (long long)p.grid_h);
  return MT_OK;
}

// What the arguments of a plane scan decide alone (`d`: "d_" for the device entry point, "" for the host one): no
// context, no device.  mtgpu_dir.h's ladder with the planes in the place of the allow bytes.
int lanes_check_args(const char *d, int rec_bytes, const void *rec, const void *frame_off, uint32_t n_frames, const void *stream_off,
                     uint32_t n_streams, const void *planes, const void *flags, const void *centres, const void *rose) {
  if (!planes) return fail(MT_ERR_INVALID, "%splanes is NULL", d);
  MT_TRY(check_rec_bytes(rec_bytes));
  MT_TRY(check_any_output(d, {{"flags", flags}, {"centres", centres}, {"rose", rose}}));
  if (n_frames > 0 && !frame_off) return fail(MT_ERR_INVALID, "%sframe_off is NULL", d);
  // per-stream planes come with the stream table, one plane for every frame without it
  if (stream_off && n_streams == 0) return fail(MT_ERR_INVALID, "%sstream_off is given and n_streams is 0", d);
  if (!stream_off && n_streams != 0) return fail(MT_ERR_INVALID, "n_streams is %u and %sstream_off is NULL", n_streams, d);
  MT_TRY(check_aligned(d, {{"frame_off", frame_off, 8}, {"stream_off", stream_off, 8}}));
  MT_TRY(check_rec(d, rec_bytes, rec));
  return check_aligned(d, {{"centres", centres, 4}, {"rose", rose, 4}});
}

// ... and of a flow-map call.
int flow_check_args(const char *d, int rec_bytes, const void *rec, const void *frame_off, uint32_t n_frames, const void *stream_off,
                    const void *flow) {
  if (!flow) return fail(MT_ERR_INVALID, "%sflow is NULL", d);
  MT_TRY(check_rec_bytes(rec_bytes));
  if (!stream_off) return fail(MT_ERR_INVALID, "%sstream_off is NULL", d);
  if (n_frames > 0 && !frame_off) return fail(MT_ERR_INVALID, "%sframe_off is NULL", d);
  MT_TRY(check_aligned(d, {{"frame_off", frame_off, 8}, {"stream_off", stream_off, 8}}));
  MT_TRY(check_rec(d, rec_bytes, rec));
  return check_aligned(d, {{"flow", flow, 4}});
}

// The plane scan of a device-resident batch on `st`.  The arguments have been validated; n_frames > 0.
// own_plan_ws: the caller's own block for the work list (a pipe's batch; ctx_plan_ws_bytes(n_frames) bytes, 256-byte
// aligned) — the launch then takes NOTHING from the context's scratch ring — and the pipe form of the launch: d_planes is
// ONE plane, d_keep one keep plane or null, no clear kernel, no stream lookup, no rose, flags and one count (the sector
// word when report_sectors) stored at system scope when `outputs_in_host_memory`.  nullptr: the ring, the resident form.
int lanes_on(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, uint64_t rebase, const uint64_t *d_off,
             const uint8_t *d_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams, const uint8_t *d_planes,
             uint8_t *d_flags, uint32_t *d_centres, mt_dir_rose *d_rose, hipStream_t st, void *own_plan_ws = nullptr,
             const uint64_t *d_keep = nullptr, int report_sectors = 0, int outputs_in_host_memory = 0) {
  mtgpu_lanes_plan lp;
  MT_TRY(lanes_plan(c->params, c->lds_max, &lp));
  mtgpu::LanesLaunch L;
  fill_batch(L, c, d_rec, rec_bytes, n_records, rebase, d_off, d_sd, n_frames, lp.lds_bytes, st);
  L.stream_off = reinterpret_cast<const unsigned long long *>(d_stream_off);
  L.n_streams = n_streams;
  L.planes = d_planes;
  L.flags = d_flags; L.centres = d_centres; L.rose = reinterpret_cast<unsigned int *>(d_rose);
  L.staged = lp.staged;
  fill_tile(L.k, c->k, mtgpu::dir_tile_words);
  L.k.clust_need = c->k.clust_need;
  if (own_plan_ws) {
    L.keep = reinterpret_cast<const unsigned long long *>(d_keep);
    L.sys_flags = (d_flags && outputs_in_host_memory) ? 1 : 0;
    L.sys_centres = (d_centres && outputs_in_host_memory) ? 1 : 0;
    L.report_sectors = report_sectors ? 1 : 0;
  }
  PlanWs ws(c, st, own_plan_ws, mtgpu::ctx_plan_ws_bytes(n_frames));
  if (ws.rc != MT_OK) return ws.rc;
  L.plan_ws = ws.p;
  if (own_plan_ws) return profiled_launch(c, st, L, mtgpu::launch_lanes_pipe, "plane pipe scan launch");
  return profiled_launch(c, st, L, mtgpu::launch_lanes_scan, "plane scan launch");
}

// The flow map of a device-resident batch on `st`.  The arguments have been validated; n_streams > 0.
int flow_on(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, uint64_t rebase, const uint64_t *d_off,
            const uint8_t *d_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams, uint32_t *d_flow,
            hipStream_t st) {
  mtgpu::FlowLaunch L;
  fill_batch(L, c, d_rec, rec_bytes, n_records, rebase, d_off, d_sd, n_frames, 0, st);
  L.stream_off = reinterpret_cast<const unsigned long long *>(d_stream_off);
  L.n_streams = n_streams;
  L.flow = d_flow;
  fill_tile(L.k, c->k, mtgpu::dir_tile_words);
  if (n_frames == 0) {                                         // only the clear
    const hipError_t e = mtgpu::launch_flow_map(L);
    return e == hipSuccess ? MT_OK : hip_fail(e, "flow map launch");
  }
  PlanWs ws(c, st, nullptr, mtgpu::ctx_plan_ws_bytes(n_frames));
  if (ws.rc != MT_OK) return ws.rc;
  L.plan_ws = ws.p;
  return profiled_launch(c, st, L, mtgpu::launch_flow_map, "flow map launch");
}

}  // namespace

namespace mtgpu {
int ctx_lanes_supported(const mtgpu_ctx *c) { return plan_ok(c, lanes_plan); }
int ctx_lanes_plane_bytes(const mtgpu_ctx *c, uint64_t *bytes) {
  mtgpu_lanes_plan lp;
  MT_TRY(lanes_plan(c->params, c->lds_max, &lp));
  *bytes = (uint64_t)lp.plane_bytes;
  return MT_OK;
}
int ctx_launch_lanes(mtgpu_ctx *c, const void *d_rec, uint64_t n_records, const uint64_t *d_off, const uint8_t *d_sd,
                     uint32_t n_frames, const uint64_t *d_keep, const uint8_t *d_plane, int report_sectors, uint8_t *d_flags,
                     uint32_t *d_count, hipStream_t st, int rec_bytes, int outputs_in_host_memory, void *plan_ws,
                     size_t plan_ws_bytes) {
  if (n_frames == 0) return MT_OK;
  if (!d_plane) return fail(MT_ERR_INVALID, "plane pipe scan without a plane");
  if (report_sectors && !d_count) return fail(MT_ERR_INVALID, "plane pipe scan: the sector report needs the batch's count array");
  MT_TRY(check_pipe_ws("plane", plan_ws, plan_ws_bytes, n_frames));
  return lanes_on(c, d_rec, rec_bytes, n_records, 0, d_off, d_sd, n_frames, nullptr, 0, d_plane, d_flags, d_count, nullptr, st, plan_ws,
                  d_keep, report_sectors ? 1 : 0, outputs_in_host_memory ? 1 : 0);
}
}  // namespace mtgpu

extern "C" {

int mtgpu_lanes_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, mtgpu_lanes_plan *out) {
  return preview(p, lds_bytes_per_workgroup, out, lanes_plan);
}

int mtgpu_scan_lanes_device(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, const uint64_t *d_frame_off,
                            const uint8_t *d_has_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams,
                            const uint8_t *d_planes, uint8_t *d_flags, uint32_t *d_centres, mt_dir_rose *d_rose, void *stream) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(lanes_check_args("d_", rec_bytes, d_rec, d_frame_off, n_frames, d_stream_off, n_streams, d_planes, d_flags, d_centres, d_rose));
  if (n_frames > 0 && n_records > 0 && !d_rec) return fail(MT_ERR_INVALID, "d_rec is NULL with n_records > 0");
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(plan_ok(c, lanes_plan));                            // a grid without a form: before any HIP call
  if (n_frames == 0) return MT_OK;
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_on_device(c, {{"d_flags", d_flags}, {"d_centres", d_centres}, {"d_rose", d_rose}}));
  MT_TRY(check_offsets_on(c, d_frame_off, n_frames, stream));
  return lanes_on(c, d_rec, rec_bytes, n_records, 0, d_frame_off, d_has_sd, n_frames, d_stream_off, n_streams, d_planes, d_flags,
                  d_centres, d_rose, static_cast<hipStream_t>(stream));
}

int mtgpu_scan_frames_lanes(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd, uint32_t n_frames,
                            const uint64_t *stream_off, uint32_t n_streams, const uint8_t *planes, uint8_t *flags, uint32_t *centres,
                            mt_dir_rose *rose) {
  MT_TRY(lanes_check_args("", MT_MV_BYTES, mv, frame_off, n_frames, stream_off, n_streams, planes, flags, centres, rose));
  MT_TRY(check_monotonic("frame_off", "frame", frame_off, n_frames));
  if (stream_off) MT_TRY(check_stream_off(stream_off, n_streams, n_frames));
  uint64_t r_begin, r_end;
  MT_TRY(check_window(mv, frame_off, n_frames, &r_begin, &r_end));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(plan_ok(c, lanes_plan));                            // a grid without a form: before anything is staged
  if (n_frames == 0) return MT_OK;

  // (with one plane for every frame stream_off is null: no room, a null device pointer)
  const size_t plane = (size_t)c->k.gh * (size_t)c->k.gw;
  Staged sg(c, c->d_misc, false, mv, r_begin, r_end, frame_off, has_sd, n_frames);
  const int i_soff = sg.in(stream_off, sizeof(uint64_t) * ((size_t)n_streams + 1));
  const int i_pl = sg.in(planes, plane * (stream_off ? (size_t)n_streams : 1u));
  const int o_fl = sg.out(flags, n_frames), o_cen = sg.out(centres, sizeof(uint32_t) * (size_t)n_frames);
  const int o_rose = sg.out(rose, sizeof(mt_dir_rose) * (size_t)n_frames);
  MT_TRY(sg.upload());
  MT_TRY(lanes_on(c, sg.d_mv(), MT_MV_BYTES, r_end, r_begin, sg.d_off(), sg.d_sd(), n_frames, sg.at<const uint64_t>(i_soff), n_streams,
                  sg.at<const uint8_t>(i_pl), sg.at<uint8_t>(o_fl), sg.at<uint32_t>(o_cen), sg.at<mt_dir_rose>(o_rose), sg.st));
  return sg.download();
}

int mtgpu_flow_map_device(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, const uint64_t *d_frame_off,
                          const uint8_t *d_has_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams,
                          uint32_t *d_flow, void *stream) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(flow_check_args("d_", rec_bytes, d_rec, d_frame_off, n_frames, d_stream_off, d_flow));
  if (n_frames > 0 && n_records > 0 && !d_rec) return fail(MT_ERR_INVALID, "d_rec is NULL with n_records > 0");
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(plan_ok(c, lanes_plan));                            // a grid without a form: before any HIP call
  if (n_streams == 0) return MT_OK;                          // no stream owns an output element
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_on_device(c, {{"d_flow", d_flow}}, " (global atomics)"));
  MT_TRY(check_offsets_on(c, d_frame_off, n_frames, stream));
  return flow_on(c, d_rec, rec_bytes, n_records, 0, d_frame_off, d_has_sd, n_frames, d_stream_off, n_streams, d_flow,
                 static_cast<hipStream_t>(stream));
}

int mtgpu_flow_map(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd, uint32_t n_frames,
                   const uint64_t *stream_off, uint32_t n_streams, uint32_t *flow) {
  MT_TRY(flow_check_args("", MT_MV_BYTES, mv, frame_off, n_frames, stream_off, flow));
  MT_TRY(check_monotonic("frame_off", "frame", frame_off, n_frames));
  MT_TRY(check_stream_off(stream_off, n_streams, n_frames));
  uint64_t r_begin, r_end;
  MT_TRY(check_window(mv, frame_off, n_frames, &r_begin, &r_end));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  MT_TRY(plan_ok(c, lanes_plan));                            // a grid without a form: before anything is staged
  if (n_streams == 0) return MT_OK;

  const size_t words = (size_t)n_streams * 8u * (size_t)c->k.gh * (size_t)c->k.gw;
  Staged sg(c, c->d_misc, false, mv, r_begin, r_end, frame_off, has_sd, n_frames);
  const int i_soff = sg.in(stream_off, sizeof(uint64_t) * ((size_t)n_streams + 1));
  const int o_flow = sg.out(flow, sizeof(uint32_t) * words);
  MT_TRY(sg.upload());
  MT_TRY(flow_on(c, sg.d_mv(), MT_MV_BYTES, r_end, r_begin, sg.d_off(), sg.d_sd(), n_frames, sg.at<const uint64_t>(i_soff), n_streams,
                 sg.at<uint32_t>(o_flow), sg.st));
  return sg.download();
}

}  // extern "C"

// ---------------------------------------------------------------- object lists (src/motion_scanner.cpp:272-294 per frame,
// then the connected components of the centres, ranked; include/mtgpu_objects.h)

namespace {

static_assert(sizeof(mt_object) == sizeof(mtgpu::ObjectWord4) && sizeof(mt_object) == 16, "mt_object is one 16-byte store");
static_assert(MT_OBJECTS_MAX == mtgpu::kObjectsMax && MT_OBJECT_TABLE_BYTES == mtgpu::kObjectTableBytes, "the kernel's limits are the ABI's");

int check_top_k(int32_t k) {
  if (k < 1 || k > MT_OBJECTS_MAX) return fail(MT_ERR_INVALID, "k is %d, outside 1 .. %d", (int)k, MT_OBJECTS_MAX);
  return MT_OK;
}

// One form: the blob scan's layout and the ranking table for k entries.  It fits or the grid is unsupported.
int objects_plan(const mt_scan_params &p, int k, int lds_max, mtgpu_objects_plan *out) {
  const int R = analysed_rows(p);
  const long long need = (long long)mtgpu::objects_lds_bytes(p.grid_w, R, k);
  if (need > (long long)lds_max)
    return fail(MT_ERR_UNSUPPORTED, "grid %dx%d: one tile of 32-bit counters for %d rows, the keep rows, one mask plane and the "
                "ranking table for %d objects (%lld bytes) do not fit %d bytes of LDS; the object scan has no banded form", p.grid_w,
                p.grid_h, R + 2, k, need, lds_max);
  const long long W = ((long long)p.grid_w + 63) / 64;
  out->lds_bytes = (int32_t)need;
  out->workgroup = mtgpu::kObjectsBlock;
  out->keep_words_per_row = (int32_t)W;
  out->keep_words_per_stream = (int32_t)(W * (long long)p.grid_h);
  return MT_OK;
}

// The object scan of a device-resident batch on `st`.  The arguments have been validated; n_frames > 0.
int objects_on(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, uint64_t rebase, const uint64_t *d_off,
               const uint8_t *d_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams, const uint64_t *d_keep,
               int32_t k, int32_t min_blob_cells, int32_t min_objects, uint8_t *d_flags, uint32_t *d_centres, uint32_t *d_blobs,
               uint32_t *d_objects, mt_object *d_list, hipStream_t st) {
  mtgpu_objects_plan op;
  MT_TRY(objects_plan(c->params, k, c->lds_max, &op));
  mtgpu::ObjLaunch L;
  fill_batch(L, c, d_rec, rec_bytes, n_records, rebase, d_off, d_sd, n_frames, op.lds_bytes, st);
  L.stream_off = reinterpret_cast<const unsigned long long *>(d_stream_off);
  L.n_streams = n_streams;
  L.keep = reinterpret_cast<const unsigned long long *>(d_keep);
  L.flags = d_flags; L.centres = d_centres; L.blobs = d_blobs; L.objects = d_objects;
  L.list = reinterpret_cast<mtgpu::ObjectWord4 *>(d_list);
  L.topk = k;
  L.obj_need = min_objects < 1 ? 1u : (unsigned int)min_objects;
  fill_tile(L.k, c->k, mtgpu::blob_tile_words);
  L.k.clust_need = c->k.clust_need;
  L.k.blob_need = min_blob_cells < 1 ? 1u : (unsigned int)min_blob_cells;
  PlanWs ws(c, st, nullptr, mtgpu::ctx_plan_ws_bytes(n_frames));
  if (ws.rc != MT_OK) return ws.rc;
  L.plan_ws = ws.p;
  return profiled_launch(c, st, L, mtgpu::launch_object_scan, "object scan launch");
}

}  // namespace

extern "C" {

int mtgpu_objects_preview(const mt_scan_params *p, int k, int lds_bytes_per_workgroup, mtgpu_objects_plan *out) {
  if (!out) return fail(MT_ERR_INVALID, "out is NULL");
  MT_TRY(check_top_k(k));
  MT_TRY(validate_params(p));
  if (lds_bytes_per_workgroup < 1024) return fail(MT_ERR_INVALID, "LDS size out of range");
  mtgpu_objects_plan pl;
  MT_TRY(objects_plan(*p, k, lds_bytes_per_workgroup, &pl));
  *out = pl;
  return MT_OK;
}

int mtgpu_scan_objects_device(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, const uint64_t *d_frame_off,
                              const uint8_t *d_has_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams,
                              const uint64_t *d_keep, int32_t k, int32_t min_blob_cells, int32_t min_objects, uint8_t *d_flags,
                              uint32_t *d_centres, uint32_t *d_blobs, uint32_t *d_objects, mt_object *d_list, void *stream) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(check_top_k(k));
  MT_TRY(check_rec_bytes(rec_bytes));
  MT_TRY(check_any_output("d_", {{"flags", d_flags}, {"centres", d_centres}, {"blobs", d_blobs}, {"objects", d_objects}, {"list", d_list}}));
  if (n_frames > 0 && !d_frame_off) return fail(MT_ERR_INVALID, "d_frame_off is NULL");
  MT_TRY(check_stream_table("d_", d_stream_off, n_streams, d_keep));
  MT_TRY(check_aligned("d_", {{"frame_off", d_frame_off, 8}, {"stream_off", d_stream_off, 8}, {"keep", d_keep, 8}}));
  if (n_frames > 0 && n_records > 0 && !d_rec) return fail(MT_ERR_INVALID, "d_rec is NULL with n_records > 0");
  MT_TRY(check_rec("d_", rec_bytes, d_rec));
  // (one 16-byte store per entry)
  MT_TRY(check_aligned("d_", {{"centres", d_centres, 4}, {"blobs", d_blobs, 4}, {"objects", d_objects, 4}, {"list", d_list, 16}}));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  mtgpu_objects_plan op;
  MT_TRY(objects_plan(c->params, k, c->lds_max, &op));       // a grid without a form: before any HIP call
  if (n_frames == 0) return MT_OK;
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_on_device(c, {{"d_keep", d_keep}, {"d_flags", d_flags}, {"d_centres", d_centres}, {"d_blobs", d_blobs},
                             {"d_objects", d_objects}, {"d_list", d_list}}));
  MT_TRY(check_offsets_on(c, d_frame_off, n_frames, stream));
  return objects_on(c, d_rec, rec_bytes, n_records, 0, d_frame_off, d_has_sd, n_frames, d_stream_off, n_streams, d_keep, k,
                    min_blob_cells, min_objects, d_flags, d_centres, d_blobs, d_objects, d_list, static_cast<hipStream_t>(stream));
}

int mtgpu_scan_frames_objects(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd, uint32_t n_frames,
                              const uint64_t *stream_off, uint32_t n_streams, const uint64_t *keep, int32_t k, int32_t min_blob_cells,
                              int32_t min_objects, uint8_t *flags, uint32_t *centres, uint32_t *blobs, uint32_t *objects,
                              mt_object *list) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(check_top_k(k));
  MT_TRY(check_any_output("", {{"flags", flags}, {"centres", centres}, {"blobs", blobs}, {"objects", objects}, {"list", list}}));
  if (n_frames > 0 && !frame_off) return fail(MT_ERR_INVALID, "frame_off is NULL");
  MT_TRY(check_stream_table("", stream_off, n_streams, keep));
  MT_TRY(check_monotonic("frame_off", "frame", frame_off, n_frames));
  if (keep) MT_TRY(check_stream_off(stream_off, n_streams, n_frames));
  uint64_t r_begin, r_end;
  MT_TRY(check_window(mv, frame_off, n_frames, &r_begin, &r_end));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  mtgpu_objects_plan op;
  MT_TRY(objects_plan(c->params, k, c->lds_max, &op));       // a grid without a form: before anything is staged
  if (n_frames == 0) return MT_OK;

  // (without a mask stream_off and keep are null and n_streams is 0: no room, null device pointers; every slot of the
  // block begins at a multiple of 256 bytes, so the device list is 16-byte aligned whatever `list` is)
  const size_t words = sizeof(uint32_t) * (size_t)n_frames;
  Staged sg(c, c->d_misc, false, mv, r_begin, r_end, frame_off, has_sd, n_frames);
  const int i_soff = sg.in(stream_off, sizeof(uint64_t) * ((size_t)n_streams + 1));
  const int i_keep = sg.in(keep, sizeof(uint64_t) * (size_t)n_streams * (size_t)c->k.gh * (size_t)c->k.W);
  const int o_fl = sg.out(flags, n_frames), o_cen = sg.out(centres, words), o_bl = sg.out(blobs, words), o_ob = sg.out(objects, words);
  const int o_list = sg.out(list, sizeof(mt_object) * (size_t)n_frames * (size_t)k);
  MT_TRY(sg.upload());
  MT_TRY(objects_on(c, sg.d_mv(), MT_MV_BYTES, r_end, r_begin, sg.d_off(), sg.d_sd(), n_frames, sg.at<const uint64_t>(i_soff), n_streams,
                    sg.at<const uint64_t>(i_keep), k, min_blob_cells, min_objects, sg.at<uint8_t>(o_fl), sg.at<uint32_t>(o_cen),
                    sg.at<uint32_t>(o_bl), sg.at<uint32_t>(o_ob), sg.at<mt_object>(o_list), sg.st));
  return sg.download();
}

}  // extern "C"

// ---------------------------------------------------------------- object headings (the object scan, then the records of
// src/motion_scanner.cpp:246-268 once more, per listed blob; include/mtgpu_headings.h)

namespace {

static_assert(sizeof(mt_heading) == 4 * sizeof(mtgpu::ObjectWord4) && sizeof(mt_heading) == 64, "mt_heading is four 16-byte stores");
static_assert(offsetof(mt_heading, records) == 32 && offsetof(mt_heading, heading) == 36 && offsetof(mt_heading, sum_dx) == 40 &&
              offsetof(mt_heading, sum_dy) == 48 && offsetof(mt_heading, reserved) == 56, "the kernel stores the fields in this order");
static_assert(MT_HEADING_TABLE_BYTES == mtgpu::kHeadingTableBytes && MT_HEADING_NONE == mtgpu::kNoHeading, "the kernel's limits are the ABI's");

// What the heading scan's own scalars decide: k, min_objects against k, the allow byte.
int check_heading_args(int32_t k, int32_t min_objects, int32_t allow) {
  MT_TRY(check_top_k(k));
  if (min_objects > k) return fail(MT_ERR_INVALID, "min_objects is %d, above k = %d", (int)min_objects, (int)k);
  if (allow < 0 || allow > 255) return fail(MT_ERR_INVALID, "allow %d outside [0,255]", (int)allow);
  return MT_OK;
}

// One form: the object scan's layout and the motion table for k entries.  It fits or the grid is unsupported.
int headings_plan(const mt_scan_params &p, int k, int lds_max, mtgpu_headings_plan *out) {
  const int R = analysed_rows(p);
  const long long need = (long long)mtgpu::headings_lds_bytes(p.grid_w, R, k);
  if (need > (long long)lds_max)
    return fail(MT_ERR_UNSUPPORTED, "grid %dx%d: one tile of 32-bit counters for %d rows, the keep rows, one mask plane, the "
                "ranking table and the motion table for %d objects (%lld bytes) do not fit %d bytes of LDS; the heading scan has no "
                "banded form", p.grid_w, p.grid_h, R + 2, k, need, lds_max);
  const long long W = ((long long)p.grid_w + 63) / 64;
  out->lds_bytes = (int32_t)need;
  out->workgroup = mtgpu::kHeadingsBlock;
  out->keep_words_per_row = (int32_t)W;
  out->keep_words_per_stream = (int32_t)(W * (long long)p.grid_h);
  return MT_OK;
}

// The heading scan of a device-resident batch on `st`.  The arguments have been validated; n_frames > 0.
int headings_on(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, uint64_t rebase, const uint64_t *d_off,
                const uint8_t *d_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams, const uint64_t *d_keep,
                int32_t k, int32_t min_blob_cells, int32_t min_objects, int32_t allow, uint8_t *d_flags, uint32_t *d_centres,
                uint32_t *d_blobs, uint32_t *d_objects, mt_object *d_list, mt_heading *d_motion, uint32_t *d_allowed, hipStream_t st) {
  mtgpu_headings_plan hp;
  MT_TRY(headings_plan(c->params, k, c->lds_max, &hp));
  mtgpu::HeadLaunch L;
  fill_batch(L, c, d_rec, rec_bytes, n_records, rebase, d_off, d_sd, n_frames, hp.lds_bytes, st);
  L.stream_off = reinterpret_cast<const unsigned long long *>(d_stream_off);
  L.n_streams = n_streams;
  L.keep = reinterpret_cast<const unsigned long long *>(d_keep);
  L.flags = d_flags; L.centres = d_centres; L.blobs = d_blobs; L.objects = d_objects;
  L.list = reinterpret_cast<mtgpu::ObjectWord4 *>(d_list);
  L.motion = reinterpret_cast<mtgpu::ObjectWord4 *>(d_motion);
  L.allowed = d_allowed;
  L.allow = (unsigned int)allow;
  L.topk = k;
  L.obj_need = min_objects < 1 ? 1u : (unsigned int)min_objects;
  fill_tile(L.k, c->k, mtgpu::blob_tile_words);
  L.k.clust_need = c->k.clust_need;
  L.k.blob_need = min_blob_cells < 1 ? 1u : (unsigned int)min_blob_cells;
  PlanWs ws(c, st, nullptr, mtgpu::ctx_plan_ws_bytes(n_frames));
  if (ws.rc != MT_OK) return ws.rc;
  L.plan_ws = ws.p;
  return profiled_launch(c, st, L, mtgpu::launch_heading_scan, "heading scan launch");
}

}  // namespace

extern "C" {

int mtgpu_headings_preview(const mt_scan_params *p, int k, int lds_bytes_per_workgroup, mtgpu_headings_plan *out) {
  if (!out) return fail(MT_ERR_INVALID, "out is NULL");
  MT_TRY(check_top_k(k));
  MT_TRY(validate_params(p));
  if (lds_bytes_per_workgroup < 1024) return fail(MT_ERR_INVALID, "LDS size out of range");
  mtgpu_headings_plan pl;
  MT_TRY(headings_plan(*p, k, lds_bytes_per_workgroup, &pl));
  *out = pl;
  return MT_OK;
}

int mtgpu_scan_headings_device(mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, const uint64_t *d_frame_off,
                               const uint8_t *d_has_sd, uint32_t n_frames, const uint64_t *d_stream_off, uint32_t n_streams,
                               const uint64_t *d_keep, int32_t k, int32_t min_blob_cells, int32_t min_objects, int32_t allow,
                               uint8_t *d_flags, uint32_t *d_centres, uint32_t *d_blobs, uint32_t *d_objects, mt_object *d_list,
                               mt_heading *d_motion, uint32_t *d_allowed, void *stream) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(check_heading_args(k, min_objects, allow));
  MT_TRY(check_rec_bytes(rec_bytes));
  MT_TRY(check_any_output("d_", {{"flags", d_flags}, {"centres", d_centres}, {"blobs", d_blobs}, {"objects", d_objects}, {"list", d_list},
                                 {"motion", d_motion}, {"allowed", d_allowed}}));
  if (n_frames > 0 && !d_frame_off) return fail(MT_ERR_INVALID, "d_frame_off is NULL");
  MT_TRY(check_stream_table("d_", d_stream_off, n_streams, d_keep));
  MT_TRY(check_aligned("d_", {{"frame_off", d_frame_off, 8}, {"stream_off", d_stream_off, 8}, {"keep", d_keep, 8}}));
  if (n_frames > 0 && n_records > 0 && !d_rec) return fail(MT_ERR_INVALID, "d_rec is NULL with n_records > 0");
  MT_TRY(check_rec("d_", rec_bytes, d_rec));
  // (one 16-byte store per list entry, four per motion entry)
  MT_TRY(check_aligned("d_", {{"centres", d_centres, 4}, {"blobs", d_blobs, 4}, {"objects", d_objects, 4}, {"allowed", d_allowed, 4},
                              {"list", d_list, 16}, {"motion", d_motion, 16}}));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  mtgpu_headings_plan hp;
  MT_TRY(headings_plan(c->params, k, c->lds_max, &hp));      // a grid without a form: before any HIP call
  if (n_frames == 0) return MT_OK;
  HIP_TRY(hipSetDevice(c->device));
  MT_TRY(check_on_device(c, {{"d_keep", d_keep}, {"d_flags", d_flags}, {"d_centres", d_centres}, {"d_blobs", d_blobs},
                             {"d_objects", d_objects}, {"d_list", d_list}, {"d_motion", d_motion}, {"d_allowed", d_allowed}}));
  MT_TRY(check_offsets_on(c, d_frame_off, n_frames, stream));
  return headings_on(c, d_rec, rec_bytes, n_records, 0, d_frame_off, d_has_sd, n_frames, d_stream_off, n_streams, d_keep, k,
                     min_blob_cells, min_objects, allow, d_flags, d_centres, d_blobs, d_objects, d_list, d_motion, d_allowed,
                     static_cast<hipStream_t>(stream));
}

int mtgpu_scan_frames_headings(mtgpu_ctx *c, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd, uint32_t n_frames,
                               const uint64_t *stream_off, uint32_t n_streams, const uint64_t *keep, int32_t k, int32_t min_blob_cells,
                               int32_t min_objects, int32_t allow, uint8_t *flags, uint32_t *centres, uint32_t *blobs,
                               uint32_t *objects, mt_object *list, mt_heading *motion, uint32_t *allowed) {
  // what the arguments alone decide comes first: these answers need neither a context nor a device
  MT_TRY(check_heading_args(k, min_objects, allow));
  MT_TRY(check_any_output("", {{"flags", flags}, {"centres", centres}, {"blobs", blobs}, {"objects", objects}, {"list", list},
                               {"motion", motion}, {"allowed", allowed}}));
  if (n_frames > 0 && !frame_off) return fail(MT_ERR_INVALID, "frame_off is NULL");
  MT_TRY(check_stream_table("", stream_off, n_streams, keep));
  MT_TRY(check_monotonic("frame_off", "frame", frame_off, n_frames));
  if (keep) MT_TRY(check_stream_off(stream_off, n_streams, n_frames));
  uint64_t r_begin, r_end;
  MT_TRY(check_window(mv, frame_off, n_frames, &r_begin, &r_end));
  if (!c) return fail(MT_ERR_INVALID, "ctx is NULL");
  mtgpu_headings_plan hp;
  MT_TRY(headings_plan(c->params, k, c->lds_max, &hp));      // a grid without a form: before anything is staged
  if (n_frames == 0) return MT_OK;

  // (without a mask stream_off and keep are null and n_streams is 0: no room, null device pointers; every slot of the
  // block begins at a multiple of 256 bytes, so the device list and motion are 16-byte aligned whatever the caller's are)
  const size_t words = sizeof(uint32_t) * (size_t)n_frames;
  Staged sg(c, c->d_misc, false, mv, r_begin, r_end, frame_off, has_sd, n_frames);
  const int i_soff = sg.in(stream_off, sizeof(uint64_t) * ((size_t)n_streams + 1));
  const int i_keep = sg.in(keep, sizeof(uint64_t) * (size_t)n_streams * (size_t)c->k.gh * (size_t)c->k.W);
  const int o_fl = sg.out(flags, n_frames), o_cen = sg.out(centres, words), o_bl = sg.out(blobs, words), o_ob = sg.out(objects, words);
  const int o_list = sg.out(list, sizeof(mt_object) * (size_t)n_frames * (size_t)k);
  const int o_mot = sg.out(motion, sizeof(mt_heading) * (size_t)n_frames * (size_t)k);
  const int o_al = sg.out(allowed, words);
  MT_TRY(sg.upload());
  MT_TRY(headings_on(c, sg.d_mv(), MT_MV_BYTES, r_end, r_begin, sg.d_off(), sg.d_sd(), n_frames, sg.at<const uint64_t>(i_soff), n_streams,
                     sg.at<const uint64_t>(i_keep), k, min_blob_cells, min_objects, allow, sg.at<uint8_t>(o_fl), sg.at<uint32_t>(o_cen),
                     sg.at<uint32_t>(o_bl), sg.at<uint32_t>(o_ob), sg.at<mt_object>(o_list), sg.at<mt_heading>(o_mot),
                     sg.at<uint32_t>(o_al), sg.st));
  return sg.download();
}

}  // extern "C"
