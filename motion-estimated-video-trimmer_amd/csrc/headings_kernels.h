// headings_kernels.h — launch interface between the C ABI (mtgpu_api.hip) and the gfx950 object-heading kernel
// (headings_kernels.hip): the object scan of objects_kernels.h and, for each of the K listed blobs, the motion of the
// counting records whose destination cell is a cell of that blob — a rose of eight sectors, the record count and the
// summed displacement (include/mtgpu_headings.h).
// Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "objects_kernels.h"

namespace mtgpu {

constexpr int kHeadingsBlock = kObjectsBlock;     // lanes per workgroup, as the object scan
constexpr int kHeadingsUnroll = kObjectsUnroll;   // independent record loads in flight per lane

// LDS of one workgroup: the object scan's layout (objects_kernels.h) and, behind the ranking table, the motion table —
// per entry 8 u32 bins, a u32 record count, a pad word, then sum_dx and sum_dy (two u64, 8-byte aligned: the layout in
// front of the table is a multiple of 8 bytes, and so is an entry).  The ONE formula: the preview, the launch check and
// the kernel's pointers rest on it.
constexpr size_t kHeadingTableBytes = 8u * 4u + 4u + 4u + 2u * 8u;     // per entry: MT_HEADING_TABLE_BYTES
constexpr int kHeadingTableWords = (int)(kHeadingTableBytes / 4u);
inline size_t headings_lds_bytes(int gw, int R, int k) { return objects_lds_bytes(gw, R, k) + (size_t)k * kHeadingTableBytes; }

// mt_heading of include/mtgpu_headings.h as the kernel stores it: FOUR 16-byte vector stores per entry.
//   [0] n[0..3]   [1] n[4..7]   [2] records, heading, sum_dx lo, hi   [3] sum_dy lo, hi, reserved lo, hi
constexpr unsigned int kNoHeading = 0xffffffffu;

struct HeadLaunch : ObjLaunch {
  ObjectWord4 *motion;                    // n_frames x topk x 4 vectors, 16-byte aligned, or null
  unsigned int *allowed;                  // n_frames words, or null
  unsigned int allow;                     // 0 .. 255: bit s admits the heading s; an entry without a heading is admitted
  // obj_need: max(1, min_objects) <= topk: flags[f] = centres[f] >= k.clust_need && allowed[f] >= obj_need
};

// Fills the non-null outputs with the answer of a frame without a blob (0; empty entries), builds the work list
// (launch_plan), then one workgroup per entry.
hipError_t launch_heading_scan(const HeadLaunch &L);

}  // namespace mtgpu
