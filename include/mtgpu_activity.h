/*
 * mtgpu_activity.h — per-stream activity maps: for every grid cell, in how many frames of a stream the cell was
 * active and in how many it was a cluster centre.  Part of the C ABI of mtgpu.h, which includes this header (include
 * either one).  Same conventions: MT_* status codes, arguments validated before anything is launched, the `*_device`
 * entry point takes device pointers and is asynchronous on `stream`, the other takes host pointers and is
 * synchronous; NO CPU fallback; no environment variables.
 *
 * What is counted (src/motion_scanner.cpp:217-295).  Let gw, gh, m = vertical_margin and vn = vectors_needed be the
 * context's (mtgpu_params_from_config).  Stream s owns frames [stream_off[s], stream_off[s + 1]), as in
 * mtgpu_merge_streams_device.  A frame CONTRIBUTES iff it has side data by the scan's rule (:219-221: has_sd[f] != 0;
 * has_sd == NULL: the frame owns at least one record — a frame with has_sd[f] != 0 and no record does contribute) and
 * its centre count, exactly what mtgpu_scan_centres_device returns for it, is >= min_centres.  min_centres == 0: every
 * frame with side data; min_centres == max(1, clusters_needed) (:288): the frames the trimmer keeps.
 *
 *   d_active[(s * gh + y) * gw + x]   contributing frames of stream s in which cell (x, y) is active: m <= y < gh - m
 *                                     (:237-238) and the cell's votes after :242-268 are >= vn (:282).  Every column
 *                                     0 .. gw - 1 (edge columns can be active, never centres).  Rows outside the
 *                                     analysed range read 0 always, also with vn == 0, where the reference treats them
 *                                     as active neighbours but never visits them.
 *   d_centre[(s * gh + y) * gw + x]   contributing frames in which the cell is one of the cells :277-292 counts,
 *                                     without the early return of :288-289: active, x in [1, gw - 2], y analysed, with
 *                                     an active 4-neighbour.  A row outside the grid is inactive; with vn == 0 and
 *                                     m > 0 the masked neighbour rows count as active, as they do in the scan.
 *   d_frames[s]                       contributing frames of stream s.
 * For every stream, the sum of its d_centre plane == the sum of the centre counts of its contributing frames.
 *
 * Any one or two of the three outputs may be NULL (never touched then); all three NULL is MT_ERR_INVALID.  Every
 * element of every non-NULL output is written: the call clears, then counts.  The maps are integers: a caller who
 * scans a recording in several batches adds them up.  They do not depend on run_frames, on the launch grid or on the
 * order in which workgroups arrive (integer adds commute).
 *
 * Kernel (csrc/activity_kernels.hip): one workgroup per RUN of consecutive entries of the scan's work list; per frame
 * one tile of 32-bit vote counters in LDS, the frame's two 64-bit mask planes, and — where they fit next to the tile —
 * two planes of LDS accumulators that collect the masks of the run's contributing frames and are added to the
 * stream's map with one global atomic per non-zero field when the run ends, the stream changes or max_run frames have
 * been collected.  Where they do not fit (4K at small margins) every contributing frame adds its masks to the map
 * directly.  A grid for which one tile and the mask planes do not fit (960x540 cells, 32767-wide grids: the grids
 * the plain scan cuts into row bands, the class mtgpu_scan_sweep_device rejects) is MT_ERR_UNSUPPORTED.
 */
#ifndef MTGPU_ACTIVITY_H
#define MTGPU_ACTIVITY_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How the activity map runs on a grid (src/motion_scanner.cpp:237-238: the analysed rows size the tile). */
typedef struct mtgpu_activity_plan {
  int32_t lds_bytes;      /* dynamic LDS per workgroup                                              */
  int32_t acc_bits;       /* width of the LDS accumulators: 32 or 16; 0 = none (every frame flushes) */
  int32_t max_run;        /* most frames one workgroup may accumulate before it must flush          */
  int32_t workgroup;      /* lanes                                                                  */
} mtgpu_activity_plan;

/*
 * The plan mtgpu_activity_map_device would pick for these parameters (the grid and the vertical margin of
 * src/motion_scanner.cpp:237-238 are all that matter) on a device with `lds_bytes_per_workgroup` of LDS per workgroup
 * (MI355X: 163840).  Pure host arithmetic: no HIP call, works without a device.  MT_ERR_INVALID: NULL / invalid
 * parameters, LDS size below 1024; MT_ERR_UNSUPPORTED (the grid is named): not even the tile and the masks fit.
 * out->lds_bytes <= lds_bytes_per_workgroup; a 16-bit plan has max_run <= 65535 (a field never wraps); a plan without
 * accumulators has max_run == 1.
 */
int mtgpu_activity_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, mtgpu_activity_plan *out);

/*
 * The activity maps (src/motion_scanner.cpp:242-292 per frame, summed per stream) of a device-resident batch;
 * asynchronous on `stream`.  d_rec / rec_bytes / n_records / d_frame_off / d_has_sd / n_frames as for
 * mtgpu_scan_centres_device (rec_bytes 40 = mt_mv, 8 = mt_mv_compact, 8-byte aligned).
 *   d_stream_off  n_streams + 1 uint64 frame offsets (device), non-decreasing, d_stream_off[n_streams] == n_frames
 *                 (PRECONDITION: a frame at or past d_stream_off[n_streams] is counted nowhere)
 *   min_centres   see above
 *   run_frames    consecutive work-list entries one workgroup accumulates in LDS before it flushes: 0 = the planner
 *                 chooses, anything else is clamped to [1, plan.max_run].  The maps are identical for every value (it
 *                 is here for the reason mtgpu_set_slices is: tests and A/B runs place the run boundaries).
 *   d_active, d_centre   n_streams * gh * gw uint32 each, or NULL;   d_frames   n_streams uint32, or NULL
 * n_frames == 0: the outputs of the n_streams streams are cleared, MT_OK.  MT_ERR_INVALID (the argument is named in
 * mtgpu_last_error) for rec_bytes outside {8, 40}, a misaligned pointer, NULL d_frame_off / d_stream_off, all outputs
 * NULL, and an output that is not memory of the context's device: the flush uses global atomics, and atomics over the
 * link to pinned host memory are not offered.  MT_ERR_UNSUPPORTED (the grid is named) as above.  Nothing is launched
 * and no output word is touched when the call fails this way.  Launch scratch (32 bytes per frame) comes from the
 * context's ring; with mtgpu_profile_enable on, the call records the same event triple as a scan launch.
 */
int mtgpu_activity_map_device(mtgpu_ctx *ctx, const void *d_rec, int rec_bytes, uint64_t n_records,
                              const uint64_t *d_frame_off, const uint8_t *d_has_sd /* may be NULL */, uint32_t n_frames,
                              const uint64_t *d_stream_off, uint32_t n_streams,
                              uint32_t min_centres, uint32_t run_frames,
                              uint32_t *d_active, uint32_t *d_centre, uint32_t *d_frames, void *stream);

/*
 * The same for a batch in HOST memory (src/motion_scanner.cpp:217-295 for every frame): copies the records the
 * offsets span, the offsets and has_sd to the device, runs the call above with the planner's run_frames, copies the
 * maps back; synchronous.  mv / frame_off / has_sd / n_frames as for mtgpu_scan_frames_centres; stream_off: n_streams
 * + 1 entries; active, centre: n_streams * gh * gw uint32 or NULL, frames: n_streams uint32 or NULL.  MT_ERR_INVALID
 * also for decreasing frame_off or stream_off and for stream_off[n_streams] != n_frames.
 */
int mtgpu_activity_map(mtgpu_ctx *ctx, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd,
                       uint32_t n_frames, const uint64_t *stream_off, uint32_t n_streams, uint32_t min_centres,
                       uint32_t *active, uint32_t *centre, uint32_t *frames);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_ACTIVITY_H */
