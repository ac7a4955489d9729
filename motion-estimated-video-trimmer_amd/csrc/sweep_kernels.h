// sweep_kernels.h — launch interface between the C ABI (mtgpu_api.hip) and the gfx950 setting-sweep kernel
// (sweep_kernels.hip): the centre counts of src/motion_scanner.cpp:272-294 for every (MV_THRESHOLD_SQ, VECTORS_NEEDED)
// pair of a study from ONE read of the records.  Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernels.h"

namespace mtgpu {

constexpr int kSweepMaxThr = 8;     // == MT_SWEEP_MAX_THRESHOLDS
constexpr int kSweepMaxVec = 8;     // == MT_SWEEP_MAX_VECTORS
constexpr int kSweepBlock = 1024;   // lanes per workgroup
constexpr int kSweepUnroll = 4;     // independent record loads in flight per lane

// LDS of one workgroup, in this order:
//   tiles    n_thr x tile_words u32     vote counters, one tile per threshold of the pass: (analysed rows + 2) x gw
//   masks    n_vec x mask_rows x W u64  activity masks of one chunk of rows, one plane per vector level
//   totals   kSweepMaxThr x kSweepMaxVec u32   the centre counts of the pass's settings
inline size_t sweep_tile_words(int gw, int analysed_rows) {
  const size_t w = (size_t)(analysed_rows + 2) * (size_t)gw;
  return (w + 3u) & ~(size_t)3u;
}
inline size_t sweep_lds_bytes(int gw, int analysed_rows, int n_thr, int n_vec, int chunk_rows) {
  const size_t W = ((size_t)gw + 63u) / 64u;
  return (size_t)n_thr * sweep_tile_words(gw, analysed_rows) * 4u + (size_t)n_vec * (size_t)(chunk_rows + 2) * W * 8u +
         (size_t)kSweepMaxThr * kSweepMaxVec * 4u;
}

// Kernel-side parameter block of one pass.
struct SweepK {
  unsigned long long thr[kSweepMaxThr];   // the pass's thresholds as integers, ascending; entries >= n_thr: ~0 (nothing passes)
  unsigned int vec[kSweepMaxVec];         // vector levels (already wrapped to uint8), caller's order
  unsigned int out_t[kSweepMaxThr];       // threshold i of the pass is the caller's threshold out_t[i]
  int n_thr, n_vec;                       // of this pass / of the call
  int shift, gw, gh, y_lo, y_hi;          // as ScanK
  int W;                                  // 64-bit words per mask row
  int tile_words;                         // sweep_tile_words
  int chunk_rows, mask_rows;              // centre rows per phase-2 chunk; chunk_rows + 2
  int sys;                                // the output is not device memory: system-scope stores
};

struct SweepLaunch : BatchLaunch {
  unsigned int *centres;                  // n_thr_all * n_vec * n_frames words, setting-major
  int n_thr_all;                          // thresholds of the call
  int thr_per_pass;                       // tiles per launch; passes = ceil(n_thr_all / thr_per_pass)
  unsigned long long thr_sorted[kSweepMaxThr];   // ascending
  unsigned int thr_index[kSweepMaxThr];          // thr_sorted[i] is the caller's threshold thr_index[i]
  SweepK k;                               // everything but thr, out_t, n_thr (set per pass)
};

// Zero-fills the whole output block, builds the work list (launch_plan), then one launch per pass.
hipError_t launch_sweep_scan(const SweepLaunch &L);

}  // namespace mtgpu
