// zones_kernels.h — launch interface between the C ABI (mtgpu_api.hip) and the gfx950 ignore-zone kernel
// (zones_kernels.hip): the centre counts of src/motion_scanner.cpp:272-294 with a per-stream keep mask ANDed into
// the active cells of the analysed rows (:282).  Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernels.h"

namespace mtgpu {

constexpr int kZoneBlock = 1024;    // lanes per workgroup
constexpr int kZoneUnroll = 4;      // independent record loads in flight per lane

// LDS of one workgroup, in this order (R = analysed rows, at least 1; W = 64-bit words per mask row):
//   tile     (R + 2) x gw u32, padded to 4 words   vote counters: the analysed rows and one halo row each side
//   keep     R x W u64                             the stream's keep words of the analysed rows; row r <-> grid row y_lo + r
//   kmask    (R + 2) x W u64                       the frame's active cells AND keep; mask row j <-> grid row y_lo - 1 + j
//   umask    (R + 2) x W u64                       the frame's active cells without the mask (written only for centres_all)
//   total    4 u32                                 [0]: the masked centre count, [1]: the unmasked one
inline size_t zone_tile_words(int gw, int R) {
  const size_t w = (size_t)(R + 2) * (size_t)gw;
  return (w + 3u) & ~(size_t)3u;
}
inline size_t zone_lds_bytes(int gw, int R) {
  const size_t W = ((size_t)gw + 63u) / 64u;
  return zone_tile_words(gw, R) * 4u + (size_t)(3 * R + 4) * W * 8u + 16u;
}

// Kernel-side parameter block.
struct ZoneK {
  unsigned long long thr;        // keep a record iff |d|^2 >= thr (ScanK::thr, :251)
  unsigned int vec_need;         // a cell is active iff votes >= vec_need (:282) and, on an analysed row, its keep bit is set
  unsigned int clust_need;       // flags[f] = centres[f] >= clust_need = max(1, clusters_needed) (:288)
  int shift, gw, gh, y_lo, y_hi; // as ScanK (y_hi >= y_lo)
  int W;                         // 64-bit words per mask row
  int R;                         // max(1, y_hi - y_lo): rows the LDS layout is sized for
  int tile_words;                // zone_tile_words
};

struct ZoneLaunch : BatchLaunch {
  const unsigned long long *stream_off;   // n_streams + 1 (pipe form: not read)
  unsigned int n_streams;
  const unsigned long long *keep;         // n_streams x gh x W, device memory (pipe form: one plane)
  unsigned char *flags;                   // n_frames bytes, device memory (pipe form: or pinned host memory), or null
  unsigned int *centres, *centres_all;    // n_frames words each, as flags, or null (pipe form: centres_all is null)
  // The pipe form (pipe.hip's staging batches): ONE plane serves every frame — no stream lookup; no clear kernel —
  // launch_plan gets the outputs and answers the frames without side data; the results are stored at system scope where
  // sys_flags / sys_centres say that the array is not device memory (a zero-copy batch's pinned block).  There is no
  // centres_all in the pipe: the pinned block has no third result array, and "what did the zones remove" is the study
  // tool's question (mtgpu_scan_zones_device, python -m mvtrim_amd.zones).  0: the form of mtgpu_scan_zones_device —
  // plain stores, sys_* must be 0.
  int pipe = 0;
  int sys_flags = 0, sys_centres = 0;
  ZoneK k;
};

// Zero-fills the non-null outputs, builds the work list (launch_plan), then one workgroup per entry.  Pipe form: no
// zero fill — the planner answers the frames without side data.
hipError_t launch_zone_scan(const ZoneLaunch &L);

}  // namespace mtgpu
