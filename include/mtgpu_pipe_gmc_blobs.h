/*
 * mtgpu_pipe_gmc_blobs.h — the compensated blob scan on the decode path: a pipe (mtgpu.h, "Host dispatcher") that runs
 * motion blobs on compensated residuals (mtgpu_gmc_blobs.h) for every batch, under the keep mask of mtgpu_pipe_zones.h
 * where the pipe carries one.  Part of the C ABI of mtgpu.h, which includes this header (include either one).  Same
 * conventions: MT_* status codes, arguments validated before anything is launched, NO CPU fallback, no environment
 * variables.
 *
 * A shaking camera in the rain: compensation alone (mtgpu_pipe_set_gmc) leaves residual noise that CLUSTERS_NEEDED
 * cannot tell from an object, a minimum blob size alone (mtgpu_pipe_set_blobs) sees the whole panned region as one
 * blob.  The residual vote lives only in the kernel's LDS tile, so no chain of pipe calls gives the pair: it is a THIRD
 * MODE of the pipe with a setter of its own.  The two single setters keep refusing each other as before.
 *
 * Semantics: mtgpu_gmc_blobs.h steps 1-5 for every frame with side data.  Under the pipe's keep plane the estimate
 * counts only records of kept cells and the active plane is the masked one — exactly as mtgpu_pipe_gmc.h and the
 * resident call define it.  flags[f] = centres >= max(1, CLUSTERS_NEEDED) AND largest >= min_blob_cells.
 *
 * Consequences.
 *  Q1. Flags and the reported count equal mtgpu_scan_frames_gmc_blobs on the same frames with the same min_blob_cells,
 *      max_shift and min_share_q8, bit for bit; with a keep plane: one stream that covers every frame, under that
 *      plane.  The count compares with its centres, its largest, or its packed info.gx / info.gy.
 *  Q2. An all-ones keep plane equals none.
 *  Q3. max_shift == 0 equals mtgpu_pipe_set_blobs(min_blob_cells, report), masked or not; under MT_PIPE_REPORT_VECTOR
 *      every count reads 0.
 *  Q4. min_blob_cells == 1 under MT_PIPE_REPORT_CENTRES or MT_PIPE_REPORT_VECTOR equals mtgpu_pipe_set_gmc with the same
 *      report: a largest blob of at least 1 cell is the same as at least 1 centre.
 *  Q5. A frame without side data reads flag 0 and count 0 under every report: the planning kernel answers it.
 *
 * The staging block of a batch has the flag bytes and ONE count array (MT_LAYOUT_CENTRES), so `report` chooses what it
 * carries.  There is no blobs or mt_gmc_info through the pipe; they stay with mtgpu_scan_gmc_blobs_device.  The largest
 * blob's box travels in an array of its own in a pipe created with MT_LAYOUT_BOXES: mtgpu_pipe_boxes.h.
 *
 * Kernel (csrc/gmc_blobs_kernels.hip, the pipe form): the compensated blob scan without its clear kernel — the planning
 * kernel answers the frames without side data — without the stream lookup and the box pass, and with system-scope result
 * stores on both of its exits where the batch's results live in pinned host memory (MT_LAYOUT_ZERO_COPY).  The keep
 * plane takes no additional LDS: the supported grids are those of mtgpu_gmc_blobs_preview.  A submit stays planning +
 * one kernel + one event, its work list in the batch's own block.
 */
#ifndef MTGPU_PIPE_GMC_BLOBS_H
#define MTGPU_PIPE_GMC_BLOBS_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The compensated blob scan for the decode path, for every batch submitted from now on.
 *   min_blob_cells >= 1   on.  max_shift must be in [0, 127] and min_share_q8 in [0, 256], otherwise MT_ERR_INVALID with
 *                         the argument named.  report: what mtgpu_batch_centres holds — MT_PIPE_REPORT_CENTRES (0),
 *                         MT_PIPE_REPORT_LARGEST (1) or MT_PIPE_REPORT_VECTOR (2, (uint16)gx | (uint16)gy << 16); the
 *                         last two need a pipe with MT_LAYOUT_CENTRES; any other value is MT_ERR_INVALID.
 *   min_blob_cells == 0   off: the pipe is bit for bit a pipe that never had it.  The other arguments are ignored and
 *                         reset.
 *   min_blob_cells < 0    MT_ERR_INVALID.
 * May be called only while no batch of the pipe is being filled or in flight: otherwise MT_ERR_BUSY, and nothing
 * changes — the same rule as mtgpu_pipe_set_keep.  MT_ERR_INVALID: pipe is NULL.  MT_ERR_UNSUPPORTED (the grid is
 * named): a grid mtgpu_gmc_blobs_preview rejects; the setting stays off and the pipe goes on as before.  A failing call
 * launches nothing.
 * Against the two single modes: turning the pair on while mtgpu_pipe_set_blobs or mtgpu_pipe_set_gmc is on is
 * MT_ERR_INVALID (the mode that is on is named: turn it off first), and nothing changes.  On a pipe in pair mode,
 * mtgpu_pipe_set_blobs(n > 0) and mtgpu_pipe_set_gmc(enable != 0) are MT_ERR_INVALID (this setter is named), and
 * nothing changes; their "off" calls stay MT_OK and leave the pair alone; mtgpu_pipe_blobs and mtgpu_pipe_gmc answer 0.
 * mtgpu_pipe_set_keep commutes with this setter; it is unchanged, so a pair pipe has a mask only on grids the masked
 * scan accepts.
 * With mtgpu_profile_enable on, a submit records one event triple, as a plain one.
 */
int mtgpu_pipe_set_gmc_blobs(mtgpu_pipe *pipe, int32_t min_blob_cells, int32_t max_shift, int32_t min_share_q8, int report);

/*
 * 1: the pipe is in pair mode, and *min_blob_cells / *max_shift / *min_share_q8 / *report (each may be NULL) receive
 * the setting; 0: it is not, nothing is written; -1: pipe is NULL.
 */
int mtgpu_pipe_gmc_blobs(const mtgpu_pipe *pipe, int32_t *min_blob_cells /* may be NULL */, int32_t *max_shift /* may be NULL */,
                         int32_t *min_share_q8 /* may be NULL */, int *report /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_PIPE_GMC_BLOBS_H */
