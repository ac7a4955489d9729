// lanes_kernels.h — launch interface between the C ABI (mtgpu_api.hip) and the gfx950 direction-plane kernels
// (lanes_kernels.hip): the direction scan of include/mtgpu_dir.h with one allow byte per grid cell in place of one per
// stream, and the flow map — the counting records per stream, sector and destination cell (include/mtgpu_lanes.h).
// Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dir_kernels.h"

namespace mtgpu {

constexpr int kLanesBlock = kDirBlock;          // lanes per workgroup
constexpr int kLanesUnroll = kDirUnroll;        // independent record loads in flight per lane
constexpr unsigned long long kLanesChunk = kDirChunk;   // records between two flushes of the lanes' packed rose counters

// LDS of one workgroup, in this order (R = analysed rows, at least 1; W = 64-bit words per mask row):
//   tile     (R + 2) x gw u32, padded to 4 words   vote counters, as dir_kernels.h
//   amask    (R + 2) x W u64                       the frame's active cells
//   rose     8 u32                                 the frame's counting records per sector
//   total    4 u32                                 [0]: the centre count; [3]: up to three head bytes of the staged plane
//   plane    R x gw bytes, padded to 16            STAGED only: rows y_lo .. y_hi - 1 of the frame's plane.  The copy keeps
//                                                  the source's phase inside a 4-byte word (it begins up to three bytes
//                                                  inside total[3]), so both sides move whole aligned words.
// The first four add up to dir_lds_bytes: the direction scan's LDS.
inline size_t lanes_plane_bytes(int gw, int R) { return ((size_t)R * (size_t)gw + 15u) & ~(size_t)15u; }
inline size_t lanes_lds_bytes(int gw, int R, bool staged) {
  return dir_lds_bytes(gw, R) + (staged ? lanes_plane_bytes(gw, R) : 0u);
}

// Kernel-side parameter block: DirK's fields (the vote is the direction scan's).
struct LanesK {
  unsigned long long thr;        // a record counts iff |d|^2 >= thr (:251) and its cell is analysed (:262)
  unsigned int vec_need;         // a cell is active iff votes >= vec_need (:282)
  unsigned int clust_need;       // flags[f] = centres[f] >= clust_need = max(1, clusters_needed) (:288)
  int shift, gw, gh, y_lo, y_hi; // as ScanK (y_hi >= y_lo)
  int W;                         // 64-bit words per mask row
  int R;                         // max(1, y_hi - y_lo): rows the LDS layout is sized for
  int tile_words;                // dir_tile_words
};

struct LanesLaunch : BatchLaunch {
  const unsigned long long *stream_off;   // n_streams + 1: stream s uses plane s; or null: ONE plane serves every frame
  unsigned int n_streams;                 // 0 with stream_off null
  const unsigned char *planes;            // n_streams (or one) x gh x gw bytes, device memory, any alignment
  unsigned char *flags;                   // n_frames bytes, device memory, or null
  unsigned int *centres;                  // n_frames words, or null
  unsigned int *rose;                     // n_frames x 8 words (mt_dir_rose), or null
  int staged;                             // 1: the plane's analysed rows are held in LDS (lds_bytes counts them)
  // The pipe form (pipe.hip's staging batches; include/mtgpu_pipe_lanes.h), launch_lanes_pipe: no clear kernel — the
  // planner gets flags and centres and answers the frames without side data; no stream lookup (`planes` is ONE plane;
  // stream_off null, n_streams 0); no rose array; the results are stored at system scope where sys_flags / sys_centres
  // say that the array is not device memory (a zero-copy batch's pinned block); `keep`: ONE plane of gh x W words in
  // device memory, or null — counting records and active cells of the analysed rows need their keep bit;
  // report_sectors: centres receives the sector word built from the frame's rose in place of the centre count.
  // launch_lanes_scan reads none of them.
  const unsigned long long *keep = nullptr;
  int sys_flags = 0, sys_centres = 0, report_sectors = 0;
  LanesK k;
};

struct FlowLaunch : BatchLaunch {
  const unsigned long long *stream_off;   // n_streams + 1
  unsigned int n_streams;
  unsigned int *flow;                     // n_streams x 8 x gh x gw words, device memory (global atomics)
  LanesK k;                               // thr, shift, the grid and the analysed rows are read
};

// Zero-fills the non-null outputs, builds the work list (launch_plan), then one workgroup per entry.
hipError_t launch_lanes_scan(const LanesLaunch &L);
// The pipe form: no fill — the planner answers the frames without side data — then one workgroup per entry of the list,
// each of which stores its frame's flag and ONE count.  Planning + one kernel.
hipError_t launch_lanes_pipe(const LanesLaunch &L);
// Zero-fills the map; then, with frames and streams, builds the work list and runs one workgroup per entry.
hipError_t launch_flow_map(const FlowLaunch &L);

}  // namespace mtgpu
