/*
 * mtgpu_pipe_blobs.h — motion blobs on the decode path: a pipe (mtgpu.h, "Host dispatcher") that applies the minimum
 * object size of mtgpu_blobs.h, with or without the keep mask of mtgpu_pipe_zones.h.  Part of the C ABI of mtgpu.h,
 * which includes this header (include either one).  Same conventions: MT_* status codes, arguments validated before
 * anything is launched, NO CPU fallback, no environment variables.
 *
 * mtgpu_scan_blobs_device tells what the trimmer WOULD keep under a minimum blob size, on a batch that is already
 * resident.  These two entry points put the rule where a recording is actually trimmed: decoder ->
 * mtgpu_batch_add_frame -> mtgpu_pipe_submit -> flags -> merge.  Centres, blobs, `largest` and the flag rule are those
 * of mtgpu_blobs.h; the keep plane, where the pipe carries one, is that of mtgpu_pipe_zones.h (ONE plane, a pipe feeds
 * one recording).
 *
 * The staging block of a batch has the flag bytes and ONE count array (MT_LAYOUT_CENTRES).  So a blob pipe reports the
 * flags and one 32-bit count per frame, chosen by `report`; there is no `blobs` and no `box` through the pipe as these
 * two entry points make it, and not both counts at once.  Those stay with mtgpu_scan_blobs_device — except the box,
 * which a pipe created with MT_LAYOUT_BOXES carries in an array of its own: mtgpu_pipe_boxes.h.
 *
 * Kernel (csrc/blobs_kernels.hip, the pipe form): the blob scan without its stream lookup and without its clear
 * kernel — the planning kernel answers the frames without side data — and with system-scope result stores, on both
 * exits of the kernel, where the batch's results live in pinned host memory (MT_LAYOUT_ZERO_COPY).  A submit stays
 * planning + one kernel + one event.  The work list lies in the batch's own block: a blob submit takes no launch
 * scratch from the context's ring.
 */
#ifndef MTGPU_PIPE_BLOBS_H
#define MTGPU_PIPE_BLOBS_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MT_PIPE_REPORT_CENTRES 0   /* mtgpu_batch_centres holds |C(f)| (masked if the pipe has a keep mask) */
#define MT_PIPE_REPORT_LARGEST 1   /* ... holds the cell count of the frame's largest blob */

/*
 * A minimum blob size for the decode path: the pipe that stands for the check_frame call in the decode loop
 * (src/motion_scanner.cpp:375-383) runs the blob scan — the centre test of src/motion_scanner.cpp:272-294, then the
 * 4-connected components of the centres — for every batch submitted from now on.
 *   min_blob_cells >= 1   the blob scan is on: mtgpu_pipe_collect's flags are
 *                         centres >= max(1, clusters_needed) AND largest >= min_blob_cells; with a keep mask
 *                         (mtgpu_pipe_set_keep) they are taken on the masked active plane.
 *   min_blob_cells == 0   off: the pipe is bit for bit a pipe that never had it, plain or masked as before.  `report`
 *                         is ignored and reset to 0.
 *   min_blob_cells < 0    MT_ERR_INVALID.
 *   report                what mtgpu_batch_centres returns — it matters only in a pipe with MT_LAYOUT_CENTRES:
 *                         MT_PIPE_REPORT_CENTRES or MT_PIPE_REPORT_LARGEST.  The choice exists because the staging block
 *                         has one count array.  MT_PIPE_REPORT_LARGEST on a pipe without MT_LAYOUT_CENTRES, and any
 *                         other value, is MT_ERR_INVALID.
 * A frame without side data reads flag 0 and count 0 under either report.
 * May be called only while no batch of the pipe is being filled or in flight (states 1 and 2; batches that are
 * collected but not yet released do not matter): otherwise MT_ERR_BUSY, and nothing changes — the same rule as
 * mtgpu_pipe_set_keep.  MT_ERR_INVALID: pipe is NULL.  MT_ERR_UNSUPPORTED (the grid is named): a grid
 * mtgpu_blobs_preview rejects; the setting stays off and the pipe goes on scanning as before.  A failing call launches
 * nothing.
 * mtgpu_pipe_set_keep and mtgpu_pipe_set_blobs commute: either order gives the same pipe, and
 * mtgpu_pipe_set_keep(pipe, NULL) on a blob pipe gives the unmasked blob scan.
 * Consequence (mtgpu_blobs.h, now from one decode pass): with MT_PIPE_REPORT_LARGEST the collected counts, handed to
 * the unchanged mtgpu_sweep_streams_device at a level L >= max(1, clusters_needed), give the segments of
 * min_blob_cells = L, bit for bit.
 * With mtgpu_profile_enable on, a blob submit records one event triple, as a plain one.
 * Compensation: this setter and mtgpu_pipe_set_gmc still refuse each other (MT_ERR_UNSUPPORTED, mtgpu_pipe_gmc.h); blobs
 * on compensated residuals are a mode of their own, mtgpu_pipe_set_gmc_blobs (mtgpu_pipe_gmc_blobs.h), and while that
 * mode is on, min_blob_cells > 0 here is MT_ERR_INVALID.
 */
int mtgpu_pipe_set_blobs(mtgpu_pipe *pipe, int32_t min_blob_cells, int report);

/*
 * 1: the pipe's submits run the blob scan (src/motion_scanner.cpp:272-294 and the components of the centres, at the
 * call site of :375-383), and *min_blob_cells / *report (each may be NULL) receive the setting; 0: they do not, nothing
 * is written; -1: pipe is NULL.
 */
int mtgpu_pipe_blobs(const mtgpu_pipe *pipe, int32_t *min_blob_cells /* may be NULL */, int *report /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_PIPE_BLOBS_H */
