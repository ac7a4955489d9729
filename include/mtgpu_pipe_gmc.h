/*
 * mtgpu_pipe_gmc.h — global-motion compensation on the decode path: a pipe (mtgpu.h, "Host dispatcher") that scans every
 * batch against each frame's dominant vector (mtgpu_gmc.h), with the estimate and the vote under the keep mask of
 * mtgpu_pipe_zones.h where the pipe carries one.  Part of the C ABI of mtgpu.h, which includes this header (include either
 * one).  Same conventions: MT_* status codes, arguments validated before anything is launched, NO CPU fallback, no
 * environment variables.
 *
 * mtgpu_scan_gmc_device tells what the trimmer WOULD keep of a shaking camera's recording, on a batch that is already
 * resident.  These two entry points put the compensation where a recording is actually trimmed: decoder ->
 * mtgpu_batch_add_frame -> mtgpu_pipe_submit -> flags -> merge.
 *
 * Why the keep mask belongs to it.  Compensation turns every static overlay into motion: a burnt-in clock or logo has
 * displacement (0, 0); after a pan of (9, 3) is subtracted its residual is (-9, -3), and it passes the threshold in every
 * compensated frame.  The vertical margin only removes full-width rows.  And an overlay that holds more records than
 * the background drags the mode to 0, so that nothing is compensated at all.  So on the decode path the estimate AND the
 * vote honour the pipe's keep plane.
 *
 * Semantics (integer, exact; an extension of mtgpu_gmc.h steps 1-5).  A pipe in compensation mode, with keep plane K
 * (mtgpu_pipe_set_keep; gh rows of W = (gw + 63) / 64 words, bit x & 63 of word x >> 6 of row y) or none, treats every
 * frame with side data as follows.
 *
 *  1. counted   a record is counted iff it passes the bounds test of src/motion_scanner.cpp:262 (0 <= dst_x >> shift <
 *               gw and m <= dst_y >> shift < gh - m) and, where the pipe has a keep plane, the keep bit of its
 *               destination cell is set.  n_in, the bins, the modes and the support test (steps 2-4 of mtgpu_gmc.h) run
 *               over the counted records only.
 *  5. vote      unchanged: EVERY record inside the bounds votes its residual into its destination cell.  The active
 *               plane is then the masked one of mtgpu_zones.h: on the analysed rows a cell is active iff it has
 *               vectors_needed votes AND its keep bit is set (vectors_needed == 0: iff its keep bit is set); rows outside
 *               the analysed range behave as in the scan.  Centres and flags are those of mtgpu_scan_gmc_device, taken
 *               on that plane.
 * A frame without side data reads flag 0 and count 0 (under either report): the planning kernel answers it, as in
 * every other pipe form.
 *
 * Consequences.
 *  P1. Without a keep plane, flags and centres equal mtgpu_scan_frames_gmc on the same frames, bit for bit.
 *  P2. An all-ones keep plane equals no keep plane.
 *  P3. max_shift == 0 equals the pipe without compensation: the plain pipe without a mask, the masked pipe
 *      (mtgpu_pipe_set_keep alone) with one.
 *  P4. With a keep plane: let (gx, gy) be what mtgpu_scan_frames_gmc reports for the frame with the records in keep-0
 *      cells removed.  The frame's centres equal what the masked pipe (no compensation) gives for the frame with
 *      (gx, gy) added to every record's src, wherever the shifted src stays inside int16.  (Consequence C of mtgpu_gmc.h
 *      under a mask.)
 *
 * The staging block of a batch has the flag bytes and ONE count array (MT_LAYOUT_CENTRES).  So a compensated pipe
 * reports the flags and one 32-bit word per frame, chosen by `report`: the centre count or the applied vector.  There
 * is no mt_gmc_info through the pipe; it stays with mtgpu_scan_gmc_device.
 *
 * Compensation together with blobs is a mode of its own, mtgpu_pipe_set_gmc_blobs (mtgpu_pipe_gmc_blobs.h); this setter
 * and mtgpu_pipe_set_blobs still refuse each other (MT_ERR_UNSUPPORTED).  Out of scope: a keep plane per
 * stream, or a keep argument on the resident mtgpu_scan_gmc_device; the row-banded grids.
 *
 * Kernel (csrc/gmc_kernels.hip, the pipe form): the compensated scan without its clear kernel — the planning kernel
 * answers the frames without side data — and with system-scope result stores where the batch's results live in pinned
 * host memory (MT_LAYOUT_ZERO_COPY), on the one exit the kernel has.  The keep plane takes no additional LDS: the keep
 * words of the analysed rows wait in the mask rows they are ANDed into, so the supported grids are those of
 * mtgpu_gmc_preview.  A submit stays planning + one kernel + one event.  The work list lies in the batch's own block: a
 * compensated submit takes no launch scratch from the context's ring.
 */
#ifndef MTGPU_PIPE_GMC_H
#define MTGPU_PIPE_GMC_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef MT_PIPE_REPORT_CENTRES
#define MT_PIPE_REPORT_CENTRES 0   /* mtgpu_batch_centres holds |C(f)| (masked if the pipe has a keep mask) */
#endif
#define MT_PIPE_REPORT_VECTOR 2   /* mtgpu_batch_centres holds (uint16)gx | (uint16)gy << 16 */

/*
 * Compensation for the decode path: the pipe that stands for the check_frame call in the decode loop
 * (src/motion_scanner.cpp:375-383) runs the compensated scan — :246-251 on the residuals of the frame's dominant vector,
 * then :262-292 — for every batch submitted from now on.
 *   enable != 0   on.  max_shift must be in [0, 127] and min_share_q8 in [0, 256] (mtgpu_gmc.h), otherwise
 *                 MT_ERR_INVALID with the argument named.  report: MT_PIPE_REPORT_CENTRES, or MT_PIPE_REPORT_VECTOR —
 *                 mtgpu_batch_centres then holds the applied vector, (uint16)gx | (uint16)gy << 16, the flag is
 *                 unchanged — which needs a pipe with MT_LAYOUT_CENTRES.  MT_PIPE_REPORT_LARGEST and any other value are
 *                 MT_ERR_INVALID.
 *   enable == 0   off: the pipe is bit for bit a pipe that never had it, plain or masked as before.  The other
 *                 arguments are ignored and reset.
 * May be called only while no batch of the pipe is being filled or in flight (states 1 and 2; batches that are
 * collected but not yet released do not matter): otherwise MT_ERR_BUSY, and nothing changes — the same rule as
 * mtgpu_pipe_set_keep.  MT_ERR_INVALID: pipe is NULL.  MT_ERR_UNSUPPORTED (the grid is named): a grid mtgpu_gmc_preview
 * rejects; the setting stays off and the pipe goes on scanning as before.  A failing call launches nothing.
 * Keep mask: mtgpu_pipe_set_keep is unchanged, so a compensated pipe has a mask only on grids the masked scan accepts
 * too; on a grid that only mtgpu_gmc_preview accepts, mtgpu_pipe_set_keep fails as before and the pipe runs unmasked
 * compensation.  mtgpu_pipe_set_keep and mtgpu_pipe_set_gmc commute.
 * Blobs: mtgpu_pipe_set_gmc(enable != 0) on a pipe with blobs on, and mtgpu_pipe_set_blobs(min_blob_cells > 0) on a pipe
 * with compensation on, are MT_ERR_UNSUPPORTED ("not together yet"), and nothing changes.
 * With mtgpu_profile_enable on, a compensated submit records one event triple, as a plain one.
 */
int mtgpu_pipe_set_gmc(mtgpu_pipe *pipe, int enable, int32_t max_shift, int32_t min_share_q8, int report);

/*
 * 1: the pipe's submits run the compensated scan (src/motion_scanner.cpp:246-292 on the residuals, at the call site of
 * :375-383), and *max_shift / *min_share_q8 / *report (each may be NULL) receive the setting; 0: they do not, nothing is
 * written; -1: pipe is NULL.
 */
int mtgpu_pipe_gmc(const mtgpu_pipe *pipe, int32_t *max_shift /* may be NULL */, int32_t *min_share_q8 /* may be NULL */,
                   int *report /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_PIPE_GMC_H */
