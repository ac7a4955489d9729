// gmc_kernels.h — launch interface between the C ABI (mtgpu_api.hip) and the gfx950 global-motion-compensated centre
// scan (gmc_kernels.hip): every frame's dominant vector is estimated from its own records, subtracted, and the
// threshold, the vote and the centres of src/motion_scanner.cpp:246-292 run on the residuals (include/mtgpu_gmc.h).
// Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernels.h"

namespace mtgpu {

constexpr int kGmcBlock = 1024;      // lanes per workgroup
constexpr int kGmcUnroll = 4;        // independent record loads in flight per lane
constexpr int kGmcMaxShift = 127;    // largest max_shift of a call
constexpr int kGmcHistBins = 256;    // bins reserved per axis: 2 * kGmcMaxShift + 1, rounded up.  The LDS size does
                                     // not depend on the call's max_shift: one plan per grid
constexpr int kGmcInfoWords = 5;     // mt_gmc_info: 20 bytes

// LDS of one workgroup, in this order (R = analysed rows, at least 1; W = 64-bit words per mask row):
//   tile     (R + 2) x gw u32, padded to 4 words   vote counters: the analysed rows and one halo row each side
//   amask    (R + 2) x W u64                       the frame's active cells; mask row j <-> grid row y_lo - 1 + j.  Dead
//                                                  until the masks are built: the pipe form keeps the keep words of the
//                                                  analysed rows in rows 1 .. R until then (keep row r <-> mask row r + 1)
//   hist     2 x kGmcHistBins u32                  hx, hy: bin v + max_shift holds the records displaced by v
//   res      8 u32                                 [0] centres, [1] n_in, [2] gx, [3] gy, [4] mode_x, [5] mode_y, [6] n_x, [7] n_y
inline size_t gmc_tile_words(int gw, int R) {
  const size_t w = (size_t)(R + 2) * (size_t)gw;
  return (w + 3u) & ~(size_t)3u;
}
inline size_t gmc_lds_bytes(int gw, int R) {
  const size_t W = ((size_t)gw + 63u) / 64u;
  return gmc_tile_words(gw, R) * 4u + (size_t)(R + 2) * W * 8u + 2u * (size_t)kGmcHistBins * 4u + 32u;
}

// Kernel-side parameter block.
struct GmcK {
  unsigned long long thr;        // keep a record iff |residual|^2 >= thr (ScanK::thr, :251)
  unsigned int vec_need;         // a cell is active iff votes >= vec_need (:282)
  unsigned int clust_need;       // flags[f] = centres[f] >= clust_need = max(1, clusters_needed) (:288)
  int shift, gw, gh, y_lo, y_hi; // as ScanK (y_hi >= y_lo)
  int W;                         // 64-bit words per mask row
  int R;                         // max(1, y_hi - y_lo): rows the LDS layout is sized for
  int tile_words;                // gmc_tile_words
  int max_shift;                 // [0, kGmcMaxShift]: displacements beyond it are in no bin
  unsigned int min_share_q8;     // [0, 256]: a mode is applied iff n * 256 >= min_share_q8 * n_in
};

struct GmcLaunch : BatchLaunch {
  unsigned char *flags;                   // n_frames bytes, device memory, or null
  unsigned int *centres;                  // n_frames words, or null
  unsigned int *info;                     // n_frames x kGmcInfoWords words (mt_gmc_info), or null
  // The pipe form (pipe.hip's staging batches; include/mtgpu_pipe_gmc.h): no clear kernel — launch_plan gets flags and
  // centres and answers the frames without side data; the results are stored at system scope where sys_flags /
  // sys_centres say that the array is not device memory (a zero-copy batch's pinned block); `keep`: ONE plane of gh x W
  // words in device memory, or null — counted records and active cells of the analysed rows need their keep bit;
  // report_vector: centres receives (uint16)gx | (uint16)gy << 16 in place of the centre count.  No info.
  // 0: the form of mtgpu_scan_gmc_device — plain stores; keep must be null, sys_* and report_vector 0.
  int pipe = 0;
  const unsigned long long *keep = nullptr;
  int sys_flags = 0, sys_centres = 0, report_vector = 0;
  GmcK k;
};

// Zero-fills the non-null outputs, builds the work list (launch_plan), then one workgroup per entry.  Pipe form: no fill —
// the planner answers the frames without side data.
hipError_t launch_gmc_scan(const GmcLaunch &L);

}  // namespace mtgpu
