// gmc_blobs_kernels.h — launch interface between the C ABI (mtgpu_api.hip) and the gfx950 compensated blob scan
// (gmc_blobs_kernels.hip): every frame's dominant vector is estimated from its own records — under a per-stream keep
// mask, from the records in kept cells — and subtracted; the threshold, the vote and the centres of
// src/motion_scanner.cpp:246-292 run on the residuals, and the centres are labelled into 4-connected components
// (include/mtgpu_gmc_blobs.h).  Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blobs_kernels.h"
#include "gmc_kernels.h"
#include "scan_kernels.h"

namespace mtgpu {

constexpr int kGmcBlobBlock = 1024;    // lanes per workgroup (a multiple of 64: a wave owns one 64-cell word of a row)
constexpr int kGmcBlobUnroll = 4;      // independent record loads in flight per lane
// What the pipe form's ONE count carries (MT_PIPE_REPORT_* of include/mtgpu.h).
constexpr int kGmcBlobReportCentres = 0, kGmcBlobReportLargest = 1, kGmcBlobReportVector = 2;

// LDS of one workgroup, in this order (R = analysed rows, at least 1; W = 64-bit words per mask row):
//   tile     (R + 2) x gw u32, padded to 4 words   vote counters of the residual vote; the labels once the masks exist
//   keep     R x W u64                             the stream's keep words of the analysed rows (no mask: ones), read by
//                                                  the masked estimate and by the masks; the centre plane later
//   amask    (R + 2) x W u64                       the frame's active cells (AND keep); mask row j <-> grid row y_lo - 1 + j
//   hist     2 x kGmcHistBins u32                  hx, hy: bin v + max_shift holds the counted records displaced by v
//   res      8 u32                                 [1] n_in, [2] gx, [3] gy, [4] mode_x, [5] mode_y, [6] n_x, [7] n_y
//   total    8 u32                                 [0] centres, [1] blobs, [2..3] the winner's key (u64), [4..7] its box
// The first three regions are the blob scan's, so the u64 key of `total` is 8-byte aligned as there.
inline size_t gmc_blobs_lds_bytes(int gw, int R) {
  return blob_lds_bytes(gw, R) + 2u * (size_t)kGmcHistBins * 4u + 32u;
}

// Kernel-side parameter block.
struct GmcBlobK {
  unsigned long long thr;        // keep a record iff |residual|^2 >= thr (ScanK::thr, :251)
  unsigned int vec_need;         // a cell is active iff votes >= vec_need (:282) and, under a mask on an analysed row, its keep bit is set
  unsigned int clust_need;       // max(1, clusters_needed) (:288)
  unsigned int blob_need;        // max(1, min_blob_cells): flags[f] = centres[f] >= clust_need && largest[f] >= blob_need
  int shift, gw, gh, y_lo, y_hi; // as ScanK (y_hi >= y_lo)
  int W;                         // 64-bit words per mask row
  int R;                         // max(1, y_hi - y_lo): rows the LDS layout is sized for
  int tile_words;                // blob_tile_words
  int max_shift;                 // [0, kGmcMaxShift]: displacements beyond it are in no bin
  unsigned int min_share_q8;     // [0, 256]: a mode is applied iff n * 256 >= min_share_q8 * n_in
};

// The six outputs of a launch, each device memory or null.
struct GmcBlobOut {
  unsigned char *flags;                   // n_frames bytes
  unsigned int *centres, *blobs, *largest;  // n_frames words each
  BlobBox *box;                           // n_frames boxes
  unsigned int *info;                     // n_frames x kGmcInfoWords words (mt_gmc_info)
};

// The ONE argument of gmc_blobs_frames_kernel: it starts the kernel-argument segment, where the kernel reads `out` a
// second time, late (gmc_blobs_kernels.hip).  The pipe form's fields stand behind `out`, so that the offsets of those
// late loads are the same in both forms.
struct GmcBlobArgs {
  const unsigned char *mv;
  const WorkItem *work;
  unsigned int item0, n_items;            // this launch serves entries [item0, n_items) of the list, one per workgroup
  GmcBlobK k;
  const unsigned long long *stream_off;
  unsigned int n_streams;
  const unsigned long long *keep;
  GmcBlobOut out;
  int sys_flags, sys_count;               // pipe form: the array is pinned host memory, stored at system scope
  int report;                             // pipe form: kGmcBlobReport*, what out.centres receives
};

struct GmcBlobLaunch : BatchLaunch {
  const unsigned long long *stream_off;   // n_streams + 1; null iff keep is null
  unsigned int n_streams;                 // 0 iff keep is null
  const unsigned long long *keep;         // n_streams x gh x W, device memory; null: no mask, no stream lookup
  unsigned char *flags;                   // n_frames bytes, device memory, or null
  unsigned int *centres, *blobs, *largest;  // n_frames words each, or null
  BlobBox *box;                           // n_frames boxes, or null
  unsigned int *info;                     // n_frames x kGmcInfoWords words (mt_gmc_info), or null
  // The pipe form (pipe.hip's staging batches; include/mtgpu_pipe_gmc_blobs.h): no clear kernel — launch_plan gets flags
  // and `centres`, the batch's ONE count array, and answers the frames without side data; the results are stored at
  // system scope where sys_flags / sys_count say that the array is not device memory; `keep` is ONE plane of gh x W
  // words or null, stream_off / n_streams null / 0; `report` (kGmcBlobReport*) chooses what `centres` receives.  blobs,
  // largest and info must be null; box is null or the batch's 8-byte aligned box array (MT_LAYOUT_BOXES: the boxed
  // kernel, which stores the box of every frame that reaches its final exit, at the scope of sys_flags).  0: the resident form — sys_* and report 0.
  int pipe = 0;
  int sys_flags = 0, sys_count = 0, report = 0;
  GmcBlobK k;
};

// Fills the non-null outputs with the answer of a frame without a blob (0; an all-0xFFFF box; a zero info), builds the
// work list (launch_plan), then one workgroup per entry.  Pipe form: no fill — the planner answers the frames without
// side data.
hipError_t launch_gmc_blob_scan(const GmcBlobLaunch &L);

}  // namespace mtgpu
