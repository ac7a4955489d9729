// scan_kernels.h — launch interface between the C ABI (mtgpu_api.hip) and the
// gfx950 scan kernels (scan_kernels.hip).  Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

namespace mtgpu {

// Kernel-side parameter block, derived on the host from mt_scan_params
// (reference cfg: include/motion_trim/motion_scanner.hpp:86-93).
struct ScanK {
  unsigned long long thr;  // keep an MV iff |d|^2 >= thr   (src/motion_scanner.cpp:251)
  int shift;               // block_shift                     (:255-256)
  int gw, gh;              // grid_w, grid_h
  int y_lo, y_hi;          // analysed rows [vertical_margin, gh - vertical_margin)  (:237-238)
  unsigned int vec_need;   // vectors_needed                  (:272)
  unsigned int clust_need; // max(1, clusters_needed)         (:288)
  int W;                   // 64-bit words per activity-mask row = ceil(gw / 64)
  int bands;               // row bands per frame (> 1: one workgroup walks them, spilling votes to a queue)
  int band_rows;           // analysed rows per band
  int fb;                  // bits per LDS vote counter: 32, or 1/2/4/8 packed
  int mode;                // 0 ADD32 (fb 32), 1 UNARY thermometer (vec_need <= fb), 2 CAS (fb 8)
  unsigned int active_min; // cell active <=> field value >= active_min
  int chunk_rows;          // centre rows per phase-2 chunk (mask buffer holds chunk_rows + 2 rows)
  int slices;              // workgroups per frame along the record array (1 = none; needs bands == 1)
  int cnt_words;           // LDS counter words per workgroup ((band_rows + 2) * gw fields, padded to 4)
  int mask_rows;           // chunk_rows + 2
  int group;               // consecutive work items per workgroup (>= 1; > 1 only with slices == 1)
  int stage_word;          // group > 1: LDS word (32-byte aligned offset behind the tile) where the workgroup parks the list
                           // entries of its 2nd .. group-th frame: 8 words each, kStageBytes in all
  int sys_flags;           // flags do not live in device memory (pinned host memory: the pipe's zero-copy staging, a caller's
                           // hipHostMalloc'ed buffer): result bytes leave with system-scope write-through stores
  int sys_centres;         // the same for the centre counts (ScanLaunch::centres)
  int early;               // 1: a frame's records are no longer read once a vote has proven its flag (scan_kernels.hip, `vote`).
                           // Per launch (launch_scan_on): 40-byte records on one ADD32 tile, slices == 1, flags only,
                           // vec_need >= 1, clust_need <= 2.  (Fills the block's tail padding: its size stays 96 bytes.)
};
static_assert(sizeof(ScanK) == 96, "ScanK is a kernel argument: `early` takes what was tail padding");

// One frame WITH motion-vector side data, as the scan's workgroups see it.  plan_frames (two small kernels ahead of
// every scan) writes the frames that have side data, in stream order, to the front of the launch's work list and
// answers every other frame on the spot (src/motion_scanner.cpp:219-221: no side data -> false): a frame without
// records never costs a workgroup slot, so no period of key frames can leave an XCD without work (the hardware deals
// workgroups to its 8 XCDs in turn).  32 bytes, read with one scalar load per workgroup.
struct WorkItem {
  unsigned long long r0, r1;   // records [r0, r1) of the frame, clamped to the batch (r0 <= r1 <= n_records)
  unsigned int f;              // frame index; kNoFrame: past the last frame with side data
  unsigned int pad[3];
};
constexpr unsigned int kNoFrame = 0xffffffffu;

// Frames per block of the planning kernels (1024 threads, `per` frames each): at most 1024 blocks; up to kPlanFused
// blocks (per == 1 then) the plan is ONE kernel.
constexpr unsigned int kPlanBlock = 1024u;
constexpr unsigned int kPlanFused = 32u;
inline unsigned int plan_per(unsigned int n_frames) {
  const unsigned long long cap = (unsigned long long)kPlanBlock * 1024ull;
  const unsigned long long per = ((unsigned long long)n_frames + cap - 1ull) / cap;
  return per > 0ull ? (unsigned int)per : 1u;
}
inline unsigned int plan_blocks(unsigned int n_frames) {
  const unsigned long long ch = (unsigned long long)kPlanBlock * plan_per(n_frames);
  return (unsigned int)(((unsigned long long)n_frames + ch - 1ull) / ch);
}
// Launch scratch of the plan: the work list (n_frames + 1 items: the last one is always kNoFrame), one count per
// planning block.
inline size_t plan_scratch_bytes(unsigned int n_frames) {
  return sizeof(WorkItem) * ((size_t)n_frames + 1u) + sizeof(unsigned int) * (size_t)plan_blocks(n_frames);
}

constexpr int kStageBytes = 64 * 32;     // LDS behind the tile for the parked entries of a grouped workgroup (group <= 64)

// What every launch over a record batch is given, whatever its kernel: the batch, the LDS it asks for, its scratch, its
// stream.  The launch structs of the scan and of its derived kernels (SweepLaunch, ActLaunch, ZoneLaunch, BlobLaunch,
// GmcLaunch, GmcBlobLaunch, DirLaunch) derive from it and add their own inputs, outputs and kernel parameter block.
// Host side only: no kernel takes a launch struct as an argument.
struct BatchLaunch {
  const unsigned char *mv;
  unsigned long long n_records;         // frame_off entries are clamped to this (in the caller's units, before `rebase`)
  unsigned long long rebase;            // records [frame_off[f], frame_off[f + 1]) live at mv + (frame_off[f] - rebase) * rec_bytes
                                        // (a host-pointer call copies only the window its offsets span); <= n_records
  const unsigned long long *frame_off;  // n_frames + 1
  const unsigned char *has_sd;          // n_frames or null
  unsigned int n_frames;
  int rec_bytes;                        // 40 = AVMotionVector records, 8 = compact {src_x,src_y,dst_x,dst_y}
  int lds_bytes;
  int lds_max;                          // device limit of dynamic LDS per workgroup (set once per kernel instantiation)
  int device;
  void *plan_ws;                        // plan_scratch_bytes(n_frames), 32-byte aligned: work list + planning counts
  hipStream_t stream;
  hipEvent_t ev_planned;                // profiling (mtgpu_profile_enable): recorded between the planning kernels and the
                                        // kernel that walks the list (a sweep: its first pass); else nullptr
};

struct ScanLaunch : BatchLaunch {
  unsigned char *flags;         // n_frames bytes; may be null when `centres` is not
  unsigned int *centres;        // n_frames words or null: every frame's centre count (0 without side data)
  unsigned int *spill_q;        // n_records words (one slot per record), only when k.bands > 1
  unsigned int *slice_ws;       // n_frames * slices * cnt_words words, only when k.slices > 1
  unsigned int *tickets;        // n_frames words (zeroed by launch_scan), only when k.slices > 1
  ScanK k;
  int block;
  unsigned long long item_chunk;  // WORKGROUPS per launch (0 = 2^30; MTGPU_ITEM_CHUNK shrinks it for tests); a workgroup scans k.group items
};

hipError_t launch_scan(const ScanLaunch &L);
// The planning kernels alone (what launch_scan runs ahead of the scan): the work list of the frames WITH side data into
// work[0 .. n_frames] and, where `flags` / `centres` are not null, the answer of every other frame.  blk_cnt: one count
// per planning block (both inside plan_scratch_bytes(n_frames)).  For launches that walk the same list with a kernel of
// their own (scalar_kernels.hip).
hipError_t launch_plan(const unsigned long long *frame_off, const unsigned char *has_sd, unsigned long long n_records,
                       unsigned long long rebase, unsigned int n_frames, unsigned char *flags, int sys_flags,
                       unsigned int *centres, int sys_centres, WorkItem *work, unsigned int *blk_cnt, hipStream_t stream);
// *first_bad (device, pre-set to 0xffffffff) = smallest f with frame_off[f] > frame_off[f + 1]
hipError_t launch_check_offsets(const unsigned long long *frame_off, unsigned int n_frames, unsigned int *first_bad,
                                hipStream_t stream);

// ---- what every launcher of a kernel over the work list does on the host

// launch_plan into the scratch of a launch: the work list at the front of plan_ws, blk_cnt behind its n_frames + 1
// entries; then the profiling event between planning and the kernel that walks the list, where there is one.
// flags / centres null: the planner answers nothing itself (the caller has cleared its outputs).
inline hipError_t plan_work_list(const unsigned long long *frame_off, const unsigned char *has_sd, unsigned long long n_records,
                                 unsigned long long rebase, unsigned int n_frames, void *plan_ws, hipStream_t stream,
                                 hipEvent_t ev_planned, unsigned char *flags, int sys_flags, unsigned int *centres,
                                 int sys_centres) {
  WorkItem *work = static_cast<WorkItem *>(plan_ws);
  unsigned int *blk_cnt = reinterpret_cast<unsigned int *>(work + (size_t)n_frames + 1u);
  hipError_t e = launch_plan(frame_off, has_sd, n_records, rebase, n_frames, flags, sys_flags, centres, sys_centres, work,
                             blk_cnt, stream);
  if (e != hipSuccess) return e;
  return ev_planned ? hipEventRecord(ev_planned, stream) : hipSuccess;
}
// The same from a launch block.  Kept out of line, one copy per launch type whoever calls it: the library's symbol list
// then does not depend on what the optimiser inlines into plan_and_launch below.
template <class Launch>
__attribute__((noinline)) hipError_t plan_work_list(const Launch &L, unsigned char *flags, int sys_flags, unsigned int *centres,
                                                    int sys_centres) {
  return plan_work_list(L.frame_off, L.has_sd, L.n_records, L.rebase, L.n_frames, L.plan_ws, L.stream, L.ev_planned, flags,
                        sys_flags, centres, sys_centres);
}

// Dynamic-LDS ceiling of a kernel: set ONCE per instantiation and device to the device maximum (host threads sharing
// an instantiation must not race each other with per-launch values).  `ready`: the instantiation's own bit set, one bit
// per device.
template <class Kern>
hipError_t raise_lds_limit_once(Kern kern, std::atomic<unsigned long long> &ready, int device, int lds_max) {
  const unsigned long long bit = 1ull << (device & 63);
  if ((ready.load(std::memory_order_acquire) & bit) == 0ull) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    if (e != hipSuccess) return e;
    ready.fetch_or(bit, std::memory_order_release);
  }
  return hipSuccess;
}

// `total` workgroups in launches of at most `chunk` (2^30: grid.x stays < 2^31): launch(first, n) starts workgroups
// [first, first + n) and is followed by hipGetLastError.
constexpr unsigned long long kGridChunk = 1ull << 30;
template <class F>
hipError_t launch_chunked(unsigned long long total, unsigned long long chunk, F launch) {
  for (unsigned long long i0 = 0; i0 < total; i0 += chunk) {
    const unsigned long long left = total - i0;
    launch(i0, (unsigned int)(left < chunk ? left : chunk));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// The launch tail of a kernel over the work list: the LDS ceiling of `kern` raised once (`ready`: the static word of the
// caller's instantiation, one per kernel instantiation), then `total` workgroups in chunks, launch(first, n) each.  The
// functor owns the argument list: it may pass arguments one by one or patch one argument block per chunk.
template <class Kern, class F>
hipError_t launch_over_list(Kern kern, std::atomic<unsigned long long> &ready, const BatchLaunch &L, unsigned long long total,
                            F launch) {
  hipError_t e = raise_lds_limit_once(kern, ready, L.device, L.lds_max);
  return e != hipSuccess ? e : launch_chunked(total, kGridChunk, launch);
}

// Blocks of 256 threads of a clear kernel over n elements (the kernels stride over what 1024 blocks leave).
inline unsigned int clear_grid(unsigned long long n) {
  const unsigned long long blocks = (n + 255ull) / 256ull;
  return (unsigned int)(blocks < 1024ull ? blocks : 1024ull);
}

// ---- the rungs every launcher over a record batch has (false: hipErrorInvalidValue)
inline bool check_batch_launch(const BatchLaunch &L) {
  return L.frame_off && L.plan_ws && ((uintptr_t)L.plan_ws & 31u) == 0u && L.rebase <= L.n_records;
}
// k: a one-tile kernel's parameter block (R tracked rows serve the analysed rows [y_lo, y_hi)); lds_need: what its
// layout takes for the block's grid.
template <class K>
bool check_rows(const K &k, int lds_bytes, int lds_max, size_t lds_need) {
  return k.R >= 1 && k.y_hi >= k.y_lo && k.R >= k.y_hi - k.y_lo && lds_bytes <= lds_max && (size_t)lds_bytes >= lds_need;
}

// The tail of a derived scan's launcher, behind its rungs.  Pipe form: the planner is handed the outputs (flags, ONE
// count array) and answers every frame without side data itself, at the outputs' scope, as in launch_scan: no clear
// kernel — planning + one kernel.  Resident form: clear(grid blocks) launches the feature's clear kernel over the frames,
// then the planner answers nothing (null outputs: they hold the clear's values already).  Then frames(rec, pipe)
// launches the instantiation for them: rec the record's bytes, 8 or 40, and pipe the form, both as constants
// (std::integral_constant), so the functor can hand them on as template arguments.
template <class Launch, class Clear, class Frames>
hipError_t plan_and_launch(const Launch &L, bool pipe, unsigned char *flags, int sys_flags, unsigned int *count, int sys_count,
                           Clear clear, Frames frames) {
  const std::integral_constant<int, 8> rec8{};
  const std::integral_constant<int, 40> rec40{};
  if (pipe) {
    hipError_t e = plan_work_list(L, flags, sys_flags, count, sys_count);
    if (e != hipSuccess) return e;
    return L.rec_bytes == 8 ? frames(rec8, std::true_type{}) : frames(rec40, std::true_type{});
  }
  clear(clear_grid(L.n_frames));
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = plan_work_list(L, nullptr, 0, nullptr, 0);
  if (e != hipSuccess) return e;
  return L.rec_bytes == 8 ? frames(rec8, std::false_type{}) : frames(rec40, std::false_type{});
}

}  // namespace mtgpu
