// blobs_kernels.h — launch interface between the C ABI (mtgpu_api.hip) and the gfx950 motion-blob kernel
// (blobs_kernels.hip): the centre cells of src/motion_scanner.cpp:272-294, with or without a per-stream keep mask
// ANDed into the active cells of the analysed rows (:282), labelled into 4-connected components per frame.
// Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernels.h"

namespace mtgpu {

constexpr int kBlobBlock = 1024;    // lanes per workgroup (a multiple of 64: a wave owns one 64-cell word of a row)
constexpr int kBlobUnroll = 4;      // independent record loads in flight per lane

// LDS of one workgroup, in this order (R = analysed rows, at least 1; W = 64-bit words per mask row):
//   tile     (R + 2) x gw u32, padded to 4 words   vote counters: the analysed rows and one halo row each side.  Dead
//                                                  once the masks exist: its first R x gw words then hold the labels,
//                                                  word r * gw + x for the cell (x, y_lo + r)
//   keep     R x W u64                             the stream's keep words of the analysed rows; row r <-> grid row
//                                                  y_lo + r.  Dead once the masks exist: the centre plane takes its
//                                                  place, R x W u64, bit x & 63 of word x >> 6 of row r
//   amask    (R + 2) x W u64                       the frame's active cells (AND keep); mask row j <-> grid row y_lo - 1 + j
//   total    8 u32                                 [0] centres, [1] blobs, [2..3] the winner's key (u64), [4..7] its box
inline size_t blob_tile_words(int gw, int R) {
  const size_t w = (size_t)(R + 2) * (size_t)gw;
  return (w + 3u) & ~(size_t)3u;
}
inline size_t blob_lds_bytes(int gw, int R) {
  const size_t W = ((size_t)gw + 63u) / 64u;
  return blob_tile_words(gw, R) * 4u + (size_t)(2 * R + 2) * W * 8u + 32u;
}

// mt_blob_box of include/mtgpu_blobs.h, as the kernel stores it (2-byte aligned, as the C struct: four 16-bit stores)
struct BlobBox { unsigned short x0, y0, x1, y1; };
// The boxed pipe form of blobs_frames_kernel and gmc_blobs_frames_kernel (MT_LAYOUT_BOXES, include/mtgpu_pipe_boxes.h) is
// chosen by their REC template argument: the record size with kRecBoxed OR-ed in.  A fifth template parameter would
// rename the four instantiations each kernel had before, and a body shared through an inlined function does not compile
// to their device code (tried: the register allocation and the address arithmetic of the record loops change); this way
// they keep both.
constexpr int kRecBoxed = 0x100;
// The same four values as the one little-endian 64-bit word the boxed pipe forms store (an 8-byte aligned array).
__host__ __device__ inline unsigned long long pack_box(unsigned int x0, unsigned int y0, unsigned int x1, unsigned int y1) {
  return (unsigned long long)(x0 & 0xffffu) | ((unsigned long long)(y0 & 0xffffu) << 16) | ((unsigned long long)(x1 & 0xffffu) << 32) |
         ((unsigned long long)(y1 & 0xffffu) << 48);
}

// Kernel-side parameter block.
struct BlobK {
  unsigned long long thr;        // keep a record iff |d|^2 >= thr (ScanK::thr, :251)
  unsigned int vec_need;         // a cell is active iff votes >= vec_need (:282) and, under a mask on an analysed row, its keep bit is set
  unsigned int clust_need;       // max(1, clusters_needed) (:288)
  unsigned int blob_need;        // max(1, min_blob_cells): flags[f] = centres[f] >= clust_need && largest[f] >= blob_need
  int shift, gw, gh, y_lo, y_hi; // as ScanK (y_hi >= y_lo)
  int W;                         // 64-bit words per mask row
  int R;                         // max(1, y_hi - y_lo): rows the LDS layout is sized for
  int tile_words;                // blob_tile_words
};

struct BlobLaunch : BatchLaunch {
  const unsigned long long *stream_off;   // n_streams + 1; null iff keep is null (pipe form: not read)
  unsigned int n_streams;                 // 0 iff keep is null (pipe form: not read)
  const unsigned long long *keep;         // n_streams x gh x W, device memory (pipe form: one plane); null: no mask, no stream lookup
  unsigned char *flags;                   // n_frames bytes, device memory (pipe form: or pinned host memory), or null
  unsigned int *centres, *blobs, *largest;  // n_frames words each, as flags, or null (pipe form: blobs is null, and at most one of centres / largest is given)
  BlobBox *box;                           // n_frames boxes, or null (pipe form: null, or the batch's 8-byte aligned box array —
                                          // the boxed kernel, which stores the box of every frame that reaches its final exit,
                                          // at the scope of sys_flags)
  // The pipe form (pipe.hip's staging batches): ONE plane serves every frame — no stream lookup; no clear kernel —
  // launch_plan gets flags and the one count array and answers the frames without side data; the results are stored at
  // system scope where sys_flags / sys_centres say that the array is not device memory (a zero-copy batch's pinned
  // block; sys_centres speaks of whichever of centres / largest is given).  The staging block has one count array: no
  // blobs, not both counts; a box only for a batch of a pipe with MT_LAYOUT_BOXES.  0: the form of mtgpu_scan_blobs_device — plain stores, sys_* must be 0.
  int pipe = 0;
  int sys_flags = 0, sys_centres = 0;
  BlobK k;
};

// Fills the non-null outputs with the answer of a frame without a blob (0; an all-0xFFFF box), builds the work list
// (launch_plan), then one workgroup per entry.  Pipe form: no fill — the planner answers the frames without side data.
hipError_t launch_blob_scan(const BlobLaunch &L);

}  // namespace mtgpu
