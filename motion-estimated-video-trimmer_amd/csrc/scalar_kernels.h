// scalar_kernels.h — launch interface between the C ABI (mtgpu_api.hip) and the gfx950 motion-scalar kernels
// (scalar_kernels.hip): the reference's per-second "motion scalar", tools/motion_scalar.cpp:61-84.
// Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernels.h"

namespace mtgpu {

// Workgroup shape of motion_scores_kernel: kScoresBlock lanes, kScoresUnroll independent record loads in flight per
// lane — one pass of a workgroup covers kScoresBlock * kScoresUnroll records (tests place frame sizes around it).
constexpr int kScoresBlock = 512;
constexpr int kScoresUnroll = 4;
// Bins per workgroup of motion_bins_kernel (one bin per lane) == frames per LDS chunk.
constexpr int kBinsBlock = 256;

struct ScoresLaunch {
  const unsigned char *mv;              // 40-byte records; frame f's records live at mv + (frame_off[f] - rebase) * 40
  unsigned long long n_records;         // frame_off entries are clamped to this (before `rebase`)
  unsigned long long rebase;
  const unsigned long long *frame_off;  // n_frames + 1
  unsigned int n_frames;
  double *scores;                       // n_frames doubles, 8-byte aligned
  unsigned int *terms;                  // n_frames words or null
  int sys_scores, sys_terms;            // the output is not device memory: system-scope write-through stores
  void *plan_ws;                        // plan_scratch_bytes(n_frames), 32-byte aligned
  hipStream_t stream;
};
// scores[f] = sum over the frame's records with motion_scale != 0 of sqrt(dx^2 + dy^2) * w * h (:75-82), terms[f] =
// the number of those records; +0.0 and 0 for a frame without records.
hipError_t launch_motion_scores(const ScoresLaunch &L);

struct BinsLaunch {
  const double *scores;                 // F
  const unsigned int *terms;            // F or null
  const double *pts;                    // F, seconds
  const unsigned long long *stream_off; // n_streams + 1 frame offsets
  unsigned int n_streams;
  unsigned int n_sec;                   // > 0
  double *acc;                          // n_streams * n_sec
  unsigned long long *bin_terms;        // n_streams * n_sec or null (needs `terms`)
  int sys_acc, sys_bin_terms;
  hipStream_t stream;
};
// acc[s * n_sec + floor(pts[f])] += scores[f] for the frames of stream s in ascending frame order (:65-66, :82)
hipError_t launch_motion_bins(const BinsLaunch &L);

}  // namespace mtgpu
