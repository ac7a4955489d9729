// api_internal.h — helpers shared by the translation units that implement the C ABI
// (mtgpu_api.hip, pipe.hip).  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtgpu.h"

namespace mtgpu {

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int hip_fail(hipError_t e, const char *what);

int ctx_device(const mtgpu_ctx *c);
// a pooled stream of the context for one staging batch (nullptr: create your own)
hipStream_t ctx_pipe_stream(mtgpu_ctx *c);
// logical -> physical HIP device (identity unless MTGPU_ALIAS_DEVICES presents more logical devices than exist)
int physical_device(int logical);
// Launch the scan for a device-resident batch on `st`.
// rec_bytes: MT_MV_BYTES (AVMotionVector records) or MT_COMPACT_BYTES (packed src/dst fields).
// flags_in_host_memory: d_flags is pinned host memory (zero-copy staging): result bytes are stored at system scope.
// d_centres: n_frames centre counts next to the flags (same memory kind as d_flags), or nullptr.
// plan_ws / plan_ws_bytes: device memory OWNED BY THE CALLER for the launch's work list (ctx_plan_ws_bytes(frames) bytes,
// 256-byte aligned; not shared with any launch that may be in flight at the same time), or nullptr / 0: stream-ordered
// scratch from the context's pool.  A pipe gives every staging batch its own: batches are submitted from many threads
// on a handful of shared streams, and their launches then allocate nothing.
int ctx_launch_scan(mtgpu_ctx *c, const void *d_mv, uint64_t n_records, const uint64_t *d_off,
                    const uint8_t *d_sd, uint32_t n_frames, uint8_t *d_flags, hipStream_t st, int rec_bytes,
                    int flags_in_host_memory, void *plan_ws, size_t plan_ws_bytes, uint32_t *d_centres = nullptr);
size_t ctx_plan_ws_bytes(uint32_t n_frames);
// Launch the masked scan (zones_kernels.hip, the pipe form) for a pipe's staging batch on `st`: as ctx_launch_scan, with
// d_keep = ONE keep plane (gh * W words, include/mtgpu_zones.h) in device memory that serves every frame of the batch.
// plan_ws / plan_ws_bytes are REQUIRED (the batch's own block): the launch takes nothing from the context's scratch
// ring.  outputs_in_host_memory: d_flags / d_centres are pinned host memory (zero-copy staging) and are stored at
// system scope; frames without side data are answered by the planning kernel at the same scope.  With
// mtgpu_profile_enable on it records the same event triple as ctx_launch_scan.  MT_ERR_UNSUPPORTED as
// mtgpu_zones_preview.
int ctx_launch_zones(mtgpu_ctx *c, const void *d_rec, uint64_t n_records, const uint64_t *d_off, const uint8_t *d_sd,
                     uint32_t n_frames, const uint64_t *d_keep, uint8_t *d_flags, uint32_t *d_centres, hipStream_t st, int rec_bytes,
                     int outputs_in_host_memory, void *plan_ws, size_t plan_ws_bytes);
// *words = uint64 words of one keep plane (gh * W) of the context's grid; MT_ERR_UNSUPPORTED (the grid is named) when
// the masked scan has no form for it.  No HIP call.
int ctx_zones_keep_words(const mtgpu_ctx *c, uint64_t *words);
// Launch the blob scan (blobs_kernels.hip, the pipe form) for a pipe's staging batch on `st`: as ctx_launch_zones, with
// d_keep = ONE keep plane in device memory or nullptr (no mask), min_blob_cells >= 1 (flags = centres >=
// max(1, clusters_needed) AND largest >= min_blob_cells) and d_count = the batch's ONE count array or nullptr, which
// receives the frame's largest blob when report_largest, else its centre count.  plan_ws / plan_ws_bytes are REQUIRED
// (the batch's own block): nothing is taken from the context's scratch ring.  outputs_in_host_memory: d_flags / d_count
// are pinned host memory and are stored at system scope, the planner's answers for frames without side data too.  With
// mtgpu_profile_enable on it records the same event triple as ctx_launch_scan.  MT_ERR_UNSUPPORTED as
// mtgpu_blobs_preview.
// d_box: nullptr, or the batch's box array (MT_LAYOUT_BOXES, include/mtgpu_pipe_boxes.h; 8-byte aligned, the same memory
// kind as d_flags): the boxed kernel runs instead and stores the largest blob's box of every frame that reaches its
// final exit — still planning + one kernel, nothing from the ring, one triple.
int ctx_launch_blobs(mtgpu_ctx *c, const void *d_rec, uint64_t n_records, const uint64_t *d_off, const uint8_t *d_sd,
                     uint32_t n_frames, const uint64_t *d_keep, int32_t min_blob_cells, int report_largest, uint8_t *d_flags,
                     uint32_t *d_count, hipStream_t st, int rec_bytes, int outputs_in_host_memory, void *plan_ws,
                     size_t plan_ws_bytes, mt_blob_box *d_box = nullptr);
// MT_OK when the blob scan has a form for the context's grid; MT_ERR_UNSUPPORTED (the grid is named) as
// mtgpu_blobs_preview otherwise.  No HIP call.
int ctx_blobs_supported(const mtgpu_ctx *c);
// Launch the compensated scan (gmc_kernels.hip, the pipe form) for a pipe's staging batch on `st`: as ctx_launch_zones,
// with d_keep = ONE keep plane in device memory or nullptr (no mask), max_shift in [0, 127], min_share_q8 in [0, 256] and
// d_count = the batch's ONE count array or nullptr, which receives (uint16)gx | (uint16)gy << 16 when report_vector
// (d_count is then required), else the frame's centre count.  plan_ws / plan_ws_bytes are REQUIRED (the batch's own
// block): nothing is taken from the context's scratch ring.  outputs_in_host_memory: d_flags / d_count are pinned host
// memory and are stored at system scope, the planner's answers for frames without side data too.  With
// mtgpu_profile_enable on it records the same event triple as ctx_launch_scan.  MT_ERR_UNSUPPORTED as mtgpu_gmc_preview.
int ctx_launch_gmc(mtgpu_ctx *c, const void *d_rec, uint64_t n_records, const uint64_t *d_off, const uint8_t *d_sd,
                   uint32_t n_frames, const uint64_t *d_keep, int32_t max_shift, int32_t min_share_q8, int report_vector,
                   uint8_t *d_flags, uint32_t *d_count, hipStream_t st, int rec_bytes, int outputs_in_host_memory, void *plan_ws,
                   size_t plan_ws_bytes);
// MT_OK when the compensated scan has a form for the context's grid; MT_ERR_UNSUPPORTED (the grid is named) as
// mtgpu_gmc_preview otherwise.  No HIP call.
int ctx_gmc_supported(const mtgpu_ctx *c);
// Launch the direction scan (dir_kernels.hip, the pipe form) for a pipe's staging batch on `st`: as ctx_launch_gmc, with
// allow in [0, 255] serving every frame and d_count = the batch's ONE count array or nullptr, which receives the sector
// word of include/mtgpu_pipe_dir.h when report_sectors (d_count is then required), else the frame's centre count.  d_keep
// = ONE keep plane in device memory or nullptr (no mask): the rose counts only records of kept cells and the active plane
// is the masked one.  plan_ws / plan_ws_bytes are REQUIRED (the batch's own block): nothing is taken from the context's
// scratch ring.  outputs_in_host_memory: d_flags / d_count are pinned host memory and are stored at system scope, the
// planner's answers for frames without side data too.  With mtgpu_profile_enable on it records the same event triple as
// ctx_launch_scan.  MT_ERR_UNSUPPORTED as mtgpu_dir_preview.
int ctx_launch_dir(mtgpu_ctx *c, const void *d_rec, uint64_t n_records, const uint64_t *d_off, const uint8_t *d_sd,
                   uint32_t n_frames, const uint64_t *d_keep, int32_t allow, int report_sectors, uint8_t *d_flags,
                   uint32_t *d_count, hipStream_t st, int rec_bytes, int outputs_in_host_memory, void *plan_ws,
                   size_t plan_ws_bytes);
// MT_OK when the direction scan has a form for the context's grid; MT_ERR_UNSUPPORTED (the grid is named) as
// mtgpu_dir_preview otherwise.  No HIP call.
int ctx_dir_supported(const mtgpu_ctx *c);
// Launch the plane scan (lanes_kernels.hip, the pipe form) for a pipe's staging batch on `st`: as ctx_launch_dir, with
// d_plane = ONE direction plane (gh * gw bytes, include/mtgpu_lanes.h) in device memory in the place of the allow byte: a
// record's byte is the one of its destination cell.  d_count receives the sector word of include/mtgpu_pipe_lanes.h when
// report_sectors (d_count is then required), else the frame's centre count.  d_keep = ONE keep plane in device memory or
// nullptr.  plan_ws / plan_ws_bytes are REQUIRED (the batch's own block): nothing is taken from the context's scratch
// ring.  outputs_in_host_memory: as ctx_launch_dir.  With mtgpu_profile_enable on it records the same event triple as
// ctx_launch_scan.  MT_ERR_UNSUPPORTED as mtgpu_lanes_preview.
int ctx_launch_lanes(mtgpu_ctx *c, const void *d_rec, uint64_t n_records, const uint64_t *d_off, const uint8_t *d_sd,
                     uint32_t n_frames, const uint64_t *d_keep, const uint8_t *d_plane, int report_sectors, uint8_t *d_flags,
                     uint32_t *d_count, hipStream_t st, int rec_bytes, int outputs_in_host_memory, void *plan_ws,
                     size_t plan_ws_bytes);
// MT_OK when the plane scan has a form for the context's grid; MT_ERR_UNSUPPORTED (the grid is named) as
// mtgpu_lanes_preview otherwise.  No HIP call.
int ctx_lanes_supported(const mtgpu_ctx *c);
// *bytes = bytes of one direction plane (gh * gw) of the context's grid; MT_ERR_UNSUPPORTED as ctx_lanes_supported.
int ctx_lanes_plane_bytes(const mtgpu_ctx *c, uint64_t *bytes);
// Launch the compensated blob scan (gmc_blobs_kernels.hip, the pipe form) for a pipe's staging batch on `st`: as
// ctx_launch_gmc, with min_blob_cells >= 1 (flags = centres >= max(1, clusters_needed) AND largest >= min_blob_cells) and
// `report` (MT_PIPE_REPORT_CENTRES / _LARGEST / _VECTOR) choosing what d_count, the batch's ONE count array or nullptr,
// receives; the last two require d_count.  plan_ws / plan_ws_bytes are REQUIRED (the batch's own block): nothing is taken
// from the context's scratch ring.  outputs_in_host_memory: d_flags / d_count are pinned host memory and are stored at
// system scope, the planner's answers for frames without side data too.  With mtgpu_profile_enable on it records the
// same event triple as ctx_launch_scan.  MT_ERR_UNSUPPORTED as mtgpu_gmc_blobs_preview.  d_box: as ctx_launch_blobs.
int ctx_launch_gmc_blobs(mtgpu_ctx *c, const void *d_rec, uint64_t n_records, const uint64_t *d_off, const uint8_t *d_sd,
                         uint32_t n_frames, const uint64_t *d_keep, int32_t max_shift, int32_t min_share_q8, int32_t min_blob_cells,
                         int report, uint8_t *d_flags, uint32_t *d_count, hipStream_t st, int rec_bytes, int outputs_in_host_memory,
                         void *plan_ws, size_t plan_ws_bytes, mt_blob_box *d_box = nullptr);
// MT_OK when the compensated blob scan has a form for the context's grid; MT_ERR_UNSUPPORTED (the grid is named) as
// mtgpu_gmc_blobs_preview otherwise.  No HIP call.
int ctx_gmc_blobs_supported(const mtgpu_ctx *c);

}  // namespace mtgpu
