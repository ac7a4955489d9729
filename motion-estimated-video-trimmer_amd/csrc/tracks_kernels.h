// tracks_kernels.h — launch interface between the C ABI (mtgpu_api.hip) and the gfx950 object-track kernels
// (tracks_kernels.hip): predecessor, age, id and track length of every list entry, include/mtgpu_tracks.h.
// Internal; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mtgpu {

constexpr int kTracksBlock = 256;                             // lanes per workgroup (four waves)
constexpr int kTracksGroup = 16;                              // lanes that share a frame: one per list entry (MT_OBJECTS_MAX)
constexpr int kTracksTile = kTracksBlock;                     // frames a workgroup takes per step: one per lane in the first scan
constexpr int kTracksWorkWords = 2;                           // words of the workspace per list entry: depth by root, ids

// mt_object of include/mtgpu_objects.h, as the kernel reads it: one 16-byte load
struct TrackObject { unsigned int cells, first, x0y0, x1y1; };

struct TracksLaunch {
  const unsigned char *flags;             // n_frames bytes: != 0 is a motion frame
  const unsigned char *has_sd;            // n_frames bytes or null: 0 on a quiet frame makes it transparent
  const TrackObject *list;                // n_frames * k entries, 16-byte aligned
  unsigned int k;                         // 1 .. 16
  unsigned int n_frames;                  // > 0, n_frames * k < 0xFFFFFFFF; stream_off entries are clamped to it
  const unsigned long long *stream_off;   // n_streams + 1
  unsigned int n_streams;                 // > 0
  unsigned int need_cells;                // max(1, min_cells)
  unsigned int max_dropout;
  unsigned int reach;                     // <= 65535
  unsigned int need_track;                // max(1, min_track)
  unsigned int *work;                     // 2 * n_frames * k words: the depth table by root, then the ids when id is null
  unsigned char *pred;                    // n_frames * k bytes or null
  unsigned int *age, *id, *len;           // n_frames * k words each or null
  unsigned int *track;                    // n_frames words or null
  unsigned char *flags_out;               // n_frames bytes or null
  hipStream_t stream;
};

// The clear kernel (empty values outside the streams, a zeroed depth table), one workgroup per stream for pred, age, id
// and the depth by root, then the finish kernel over all frames for len, track and flags_out.
hipError_t launch_tracks(const TracksLaunch &L);

}  // namespace mtgpu
