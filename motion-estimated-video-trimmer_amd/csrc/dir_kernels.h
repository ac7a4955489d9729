// dir_kernels.h — launch interface between the C ABI (mtgpu_api.hip) and the gfx950 direction-filter kernel
// (dir_kernels.hip): the centre counts of src/motion_scanner.cpp:272-294 from the votes of the records whose sector is
// allowed (include/mtgpu_dir.h), and the per-frame rose of the counting records.  Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernels.h"

namespace mtgpu {

constexpr int kDirBlock = 1024;     // lanes per workgroup
constexpr int kDirUnroll = 4;       // independent record loads in flight per lane
// Records a workgroup streams between two flushes of the lanes' packed rose counters (eight 8-bit fields).  A lane
// sees at most kDirChunk / kDirBlock records of the steps, one of the head peel and one odd last record: 130 < 256.
constexpr unsigned long long kDirChunk = 128ull * kDirBlock;
static_assert(kDirChunk / kDirBlock + 2 < 256, "a lane's 8-bit rose field must not wrap between two flushes");
static_assert((kDirChunk / kDirBlock + 2) * 64 < 65536, "a wave's 16-bit partial sums must not wrap");

// LDS of one workgroup, in this order (R = analysed rows, at least 1; W = 64-bit words per mask row):
//   tile     (R + 2) x gw u32, padded to 4 words   vote counters: the analysed rows and one halo row each side
//   amask    (R + 2) x W u64                       the frame's active cells; mask row j <-> grid row y_lo - 1 + j.  Dead
//                                                  until the masks are built: the pipe form keeps the keep words of the
//                                                  analysed rows in rows 1 .. R until then (keep row r <-> mask row r + 1)
//   total    4 u32                                 [0]: the centre count
//   rose     8 u32                                 the frame's counting records per sector
inline size_t dir_tile_words(int gw, int R) {
  const size_t w = (size_t)(R + 2) * (size_t)gw;
  return (w + 3u) & ~(size_t)3u;
}
inline size_t dir_lds_bytes(int gw, int R) {
  const size_t W = ((size_t)gw + 63u) / 64u;
  return dir_tile_words(gw, R) * 4u + (size_t)(R + 2) * W * 8u + 16u + 32u;
}

// Kernel-side parameter block.
struct DirK {
  unsigned long long thr;        // a record counts iff |d|^2 >= thr (ScanK::thr, :251) and its cell is analysed (:262)
  unsigned int vec_need;         // a cell is active iff votes >= vec_need (:282)
  unsigned int clust_need;       // flags[f] = centres[f] >= clust_need = max(1, clusters_needed) (:288)
  int shift, gw, gh, y_lo, y_hi; // as ScanK (y_hi >= y_lo)
  int W;                         // 64-bit words per mask row
  int R;                         // max(1, y_hi - y_lo): rows the LDS layout is sized for
  int tile_words;                // dir_tile_words
};

struct DirLaunch : BatchLaunch {
  const unsigned long long *stream_off;   // n_streams + 1, or null: `allow` serves every frame
  unsigned int n_streams;
  const unsigned char *allows;            // n_streams bytes, device memory, or null (then stream_off is null, n_streams 0)
  unsigned int allow;                     // 0 .. 255; read only without `allows`
  unsigned char *flags;                   // n_frames bytes, device memory, or null
  unsigned int *centres;                  // n_frames words, or null
  unsigned int *rose;                     // n_frames x 8 words (mt_dir_rose), or null
  // The pipe form (pipe.hip's staging batches; include/mtgpu_pipe_dir.h): no clear kernel — launch_plan gets flags and
  // centres and answers the frames without side data; no stream lookup (`allow` serves every frame; allows / stream_off
  // null); the results are stored at system scope where sys_flags / sys_centres say that the array is not device memory
  // (a zero-copy batch's pinned block); `keep`: ONE plane of gh x W words in device memory, or null — counting records
  // and active cells of the analysed rows need their keep bit; report_sectors: centres receives the sector word built
  // from the frame's rose in place of the centre count.  No rose array.
  // 0: the form of mtgpu_scan_dir_device — plain stores; keep must be null, sys_* and report_sectors 0.
  int pipe = 0;
  const unsigned long long *keep = nullptr;
  int sys_flags = 0, sys_centres = 0, report_sectors = 0;
  DirK k;
};

// Zero-fills the non-null outputs, builds the work list (launch_plan), then one workgroup per entry.  Pipe form: no fill —
// the planner answers the frames without side data.
hipError_t launch_dir_scan(const DirLaunch &L);

}  // namespace mtgpu
