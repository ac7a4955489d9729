// objects_kernels.h — launch interface between the C ABI (mtgpu_api.hip) and the gfx950 object-list kernel
// (objects_kernels.hip): the blobs of blobs_kernels.h, with or without a per-stream keep mask, ranked by size; the K
// largest of every frame leave the kernel with their boxes, and a count of the blobs of a minimum size.
// Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blobs_kernels.h"

namespace mtgpu {

constexpr int kObjectsBlock = kBlobBlock;     // lanes per workgroup, as the blob scan
constexpr int kObjectsUnroll = kBlobUnroll;   // independent record loads in flight per lane
constexpr int kObjectsMax = 16;               // MT_OBJECTS_MAX: list entries per frame

// LDS of one workgroup: the blob scan's layout (blobs_kernels.h: tile, keep, amask, total) and, behind `total`, the
// ranking table of blob_rank.h — k keys (u64), then k boxes (4 u32 each).  blob_lds_bytes is a multiple of 16, so the
// keys are 8-byte aligned.  The ONE formula: the preview, the launch check and the kernel's pointers rest on it.
constexpr size_t kObjectTableBytes = 8u + 16u;     // per entry: MT_OBJECT_TABLE_BYTES
inline size_t objects_lds_bytes(int gw, int R, int k) { return blob_lds_bytes(gw, R) + (size_t)k * kObjectTableBytes; }

// mt_object of include/mtgpu_objects.h as the kernel stores it: ONE 16-byte vector store per entry.
//   x: cells   y: first   z: x0 | y0 << 16   w: x1 | y1 << 16       (little-endian: the struct's field order)
typedef unsigned int ObjectWord4 __attribute__((ext_vector_type(4)));
constexpr unsigned int kNoObjectFirst = 0xffffffffu, kNoObjectBox = 0xffffffffu;

struct ObjLaunch : BatchLaunch {
  const unsigned long long *stream_off;   // n_streams + 1; null iff keep is null
  unsigned int n_streams;                 // 0 iff keep is null
  const unsigned long long *keep;         // n_streams x gh x W, device memory; null: no mask, no stream lookup
  unsigned char *flags;                   // n_frames bytes, device memory, or null
  unsigned int *centres, *blobs, *objects;  // n_frames words each, or null
  ObjectWord4 *list;                      // n_frames x topk entries, 16-byte aligned, or null
  int topk;                               // 1 .. kObjectsMax
  unsigned int obj_need;                  // max(1, min_objects): flags[f] = centres[f] >= k.clust_need && objects[f] >= obj_need
  BlobK k;                                // blob_need = max(1, min_blob_cells): what objects[f] counts
};

// Fills the non-null outputs with the answer of a frame without a blob (0; empty entries), builds the work list
// (launch_plan), then one workgroup per entry.
hipError_t launch_object_scan(const ObjLaunch &L);

}  // namespace mtgpu
