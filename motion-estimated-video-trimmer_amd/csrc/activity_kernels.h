// activity_kernels.h — launch interface between the C ABI (mtgpu_api.hip) and the gfx950 activity-map kernels
// (activity_kernels.hip): per stream and grid cell, the frames in which the cell was active / a centre
// (src/motion_scanner.cpp:242-292).  Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernels.h"

namespace mtgpu {

constexpr int kActBlock = 1024;    // lanes per workgroup
constexpr int kActUnroll = 4;      // independent record loads in flight per lane

// LDS of one workgroup, in this order (R = analysed rows, at least 1; W = 64-bit words per mask row):
//   tile     (R + 2) x gw u32, padded to 4 words   vote counters: the analysed rows and one halo row each side
//   acc_a    R x gwp fields of acc_bits            active-cell accumulator, gwp = gw rounded up to 4   (acc_bits > 0)
//   acc_c    R x gwp fields of acc_bits            centre accumulator                                    (acc_bits > 0)
//   amask    (R + 2) x W u64                       the frame's active cells; mask row j <-> grid row y_lo - 1 + j
//   cmask    R x W u64                             the frame's centres; row r <-> grid row y_lo + r
//   total    4 u32                                 [0]: the frame's centre count
inline size_t act_tile_words(int gw, int R) {
  const size_t w = (size_t)(R + 2) * (size_t)gw;
  return (w + 3u) & ~(size_t)3u;
}
inline int act_gwp(int gw) { return (gw + 3) & ~3; }
inline size_t act_acc_plane_bytes(int gw, int R, int acc_bits) { return (size_t)R * (size_t)act_gwp(gw) * (size_t)(acc_bits / 8); }
inline size_t act_lds_bytes(int gw, int R, int acc_bits) {
  const size_t W = ((size_t)gw + 63u) / 64u;
  return act_tile_words(gw, R) * 4u + 2u * act_acc_plane_bytes(gw, R, acc_bits) + (size_t)(2 * R + 2) * W * 8u + 16u;
}

// Kernel-side parameter block.
struct ActK {
  unsigned long long thr;        // keep a record iff |d|^2 >= thr (ScanK::thr, :251)
  unsigned int vec_need;         // a cell is active iff votes >= vec_need (:282)
  unsigned int min_centres;      // a frame contributes iff its centre count >= min_centres
  int shift, gw, gh, y_lo, y_hi; // as ScanK (y_hi >= y_lo)
  int W;                         // 64-bit words per mask row
  int R;                         // max(1, y_hi - y_lo): rows the LDS layout is sized for
  int tile_words;                // act_tile_words
  int gwp;                       // act_gwp
  int run;                       // work-list entries per workgroup (>= 1)
  int max_run;                   // contributing frames the accumulators may hold (>= 1)
};

struct ActLaunch : BatchLaunch {            // (plan_ws is unused when n_frames == 0)
  const unsigned long long *stream_off;   // n_streams + 1
  unsigned int n_streams;
  unsigned int *active, *centre, *frames; // device memory; any may be null
  ActK k;
  int acc_bits;                           // 32, 16 or 0
};

// Clears the non-null outputs, builds the work list (launch_plan), then one workgroup per run of k.run entries.
hipError_t launch_activity_map(const ActLaunch &L);

}  // namespace mtgpu
