// persist_kernels.h — launch interface between the C ABI (mtgpu_api.hip) and the gfx950 temporal-persistence kernels
// (persist_kernels.hip): run lengths of motion frames per stream, include/mtgpu_persist.h.
// Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mtgpu {

constexpr int kPersistBlock = 256;                            // lanes per workgroup (four waves)
constexpr int kPersistItems = 4;                              // consecutive frames a lane owns in a tile
constexpr int kPersistTile = kPersistBlock * kPersistItems;   // frames a workgroup takes per step

// mt_blob_box of include/mtgpu_blobs.h, as the kernel reads it (2-byte aligned, as the C struct: four 16-bit loads)
struct PersistBox { unsigned short x0, y0, x1, y1; };

struct PersistLaunch {
  const unsigned char *flags;             // n_frames bytes: != 0 is a motion frame
  const unsigned char *has_sd;            // n_frames bytes or null: 0 on a quiet frame makes it transparent
  const PersistBox *box;                  // n_frames boxes or null: no link test
  unsigned int n_frames;                  // > 0; stream_off entries are clamped to it
  const unsigned long long *stream_off;   // n_streams + 1
  unsigned int n_streams;                 // > 0
  unsigned int need;                      // max(1, min_run)
  unsigned int max_dropout;
  unsigned int reach;                     // <= 65535
  unsigned int *work;                     // n_frames words: holds pos between the two walks when pos is null
  unsigned char *flags_out;               // n_frames bytes or null
  unsigned int *run, *pos;                // n_frames words each or null
  hipStream_t stream;
};

// One small kernel clears the frames outside [stream_off[0], stream_off[n_streams]) in the non-null outputs, then one
// workgroup per stream walks it forwards (pos) and backwards (run, flags_out).
hipError_t launch_persist(const PersistLaunch &L);

}  // namespace mtgpu
