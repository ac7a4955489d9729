/*
 * mtgpu_pipe_dir.h — the direction filter on the decode path: a pipe (mtgpu.h, "Host dispatcher") in which a record
 * votes only if the sector of its displacement is allowed (mtgpu_dir.h), under the keep mask of mtgpu_pipe_zones.h where
 * the pipe carries one.  Part of the C ABI of mtgpu.h, which includes this header (include either one).  Same
 * conventions: MT_* status codes, arguments validated before anything is launched, NO CPU fallback, no environment
 * variables.
 *
 * mtgpu_scan_dir_device and `python -m mvtrim_amd.direction` tell which allow byte a camera wants, on a batch that is
 * already resident.  These two entry points put the rule where a recording is actually trimmed: decoder ->
 * mtgpu_batch_add_frame -> mtgpu_pipe_submit -> flags -> merge.
 *
 * Why the keep mask belongs to it.  A conveyor that should not vote is handled by the byte, a burnt-in clock by the
 * mask, and real cameras have both.
 *
 * Semantics (integer, exact; an extension of mtgpu_dir.h steps 1-4).  A pipe in direction mode has allow byte `a` and a
 * keep plane K (mtgpu_pipe_set_keep; gh rows of W = (gw + 63) / 64 words, bit x & 63 of word x >> 6 of row y) or none.
 * It treats every frame with side data as follows.
 *
 *  1. counts    a record COUNTS iff it passes the bounds test and the threshold of mtgpu_dir.h step 1 and, where the
 *               pipe has a keep plane, the keep bit of its destination cell is set.
 *  2. n[k]      the number of counting records of sector k, for every k, WHATEVER `a` says.  Records without a sector
 *               are in no n[k].
 *  3. vote      every record that passes step 1 WITHOUT the keep condition, and passes the direction test under `a`,
 *               votes for its destination cell.  A record without a sector always passes.
 *  4. active    the active plane is the masked one of mtgpu_zones.h: on the analysed rows a cell is active iff it has
 *               vectors_needed votes AND its keep bit is set (vectors_needed == 0: iff its keep bit is set); rows
 *               outside the analysed range behave as in the scan.  Centres and flags are then those of
 *               mtgpu_scan_dir_device, taken on that plane.  (An implementation may skip the vote of a record in a
 *               keep-0 cell: the cell is inactive whatever its votes, so the result is the same.)
 *  5. MT_PIPE_REPORT_CENTRES   mtgpu_batch_centres holds the centre count.
 *  6. MT_PIPE_REPORT_SECTORS   mtgpu_batch_centres holds one word, the frame's SECTOR WORD:
 *               bits 0 .. 7     the present byte: bit k is set iff n[k] >= 1
 *               bits 8 .. 10    k*, the smallest k whose n[k] is maximal; 0 when every n[k] is 0
 *               bits 11 .. 31   min(n[k*], 2^21 - 1)
 *               A frame without a counting moving record reads 0.  The flag is the same under either report.
 * A frame without side data reads flag 0 and word 0 (under either report): the planning kernel answers it, as in every
 * other pipe form.
 *
 * Consequences (what the tests hold).
 *  D1. Without a keep plane, flags and centres equal mtgpu_scan_frames_dir with the scalar `allow` on the same frames,
 *      bit for bit, and the sector word equals the word derived from its rose.
 *  D2. An all-ones keep plane equals no keep plane.
 *  D3. allow == 0xFF with the centre report equals the pipe without the mode: the plain pipe without a mask, the masked
 *      pipe (mtgpu_pipe_set_keep alone) with one.
 *  D4. With a keep plane: the centres equal what the masked pipe (no direction) gives for the frames with every record
 *      of a forbidden sector removed; the sector word equals the word derived from the resident rose of the frames with
 *      the records of keep-0 cells removed.
 *  D5. The sector word does not depend on allow.
 *
 * The staging block of a batch has the flag bytes and ONE count array (MT_LAYOUT_CENTRES).  So a direction pipe reports
 * the flags and one 32-bit word per frame, chosen by `report`.  There is no mt_dir_rose through the pipe; the full rose
 * stays with mtgpu_scan_dir_device.
 *
 * Out of scope: a full mt_dir_rose array through the pipe (a layout bit of its own, as MT_LAYOUT_BOXES was); per-stream
 * allow bytes on a pipe; a per-cell allow plane (that one is in mtgpu_pipe_lanes.h); direction together with blobs, compensation or the compensated blob
 * scan — the setters refuse each other (MT_ERR_UNSUPPORTED, "not together yet"); a keep argument on the resident
 * mtgpu_scan_dir_device; the row-banded grids.
 *
 * Kernel (csrc/dir_kernels.hip, the pipe form): the direction scan without its clear kernel — the planning kernel
 * answers the frames without side data — without the stream lookup, and with system-scope result stores where the
 * batch's results live in pinned host memory (MT_LAYOUT_ZERO_COPY), on the one exit the kernel has.  Lane 0 builds the
 * sector word from the eight rose words in LDS.  The keep plane takes no additional LDS: the keep words of the analysed
 * rows wait in the mask rows they are ANDed into, so the supported grids are exactly those of mtgpu_dir_preview.  A
 * submit stays planning + one kernel + one event.  The work list lies in the batch's own block: a direction submit takes
 * no launch scratch from the context's ring.
 */
#ifndef MTGPU_PIPE_DIR_H
#define MTGPU_PIPE_DIR_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef MT_PIPE_REPORT_CENTRES
#define MT_PIPE_REPORT_CENTRES 0   /* mtgpu_batch_centres holds |C(f)| (masked if the pipe has a keep mask) */
#endif
#define MT_PIPE_REPORT_SECTORS 3   /* mtgpu_batch_centres holds the frame's sector word (above) */

/*
 * The direction filter for the decode path: the pipe that stands for the check_frame call in the decode loop
 * (src/motion_scanner.cpp:375-383) runs the direction scan for every batch submitted from now on.
 *   enable != 0   on.  allow must be in 0 .. 255, otherwise MT_ERR_INVALID with the argument named.  report:
 *                 MT_PIPE_REPORT_CENTRES, or MT_PIPE_REPORT_SECTORS — mtgpu_batch_centres then holds the sector word, the
 *                 flag is unchanged — which needs a pipe with MT_LAYOUT_CENTRES.  Any other value is MT_ERR_INVALID.
 *   enable == 0   off: the pipe is bit for bit a pipe that never had it, plain or masked as before.  The other
 *                 arguments are ignored and reset.
 * May be called only while no batch of the pipe is being filled or in flight (states 1 and 2; batches that are
 * collected but not yet released do not matter): otherwise MT_ERR_BUSY, and nothing changes — the same rule as
 * mtgpu_pipe_set_keep.  MT_ERR_INVALID: pipe is NULL.  MT_ERR_UNSUPPORTED (the grid is named): a grid mtgpu_dir_preview
 * rejects; the setting stays off and the pipe goes on scanning as before.  A failing call launches nothing.
 * Keep mask: mtgpu_pipe_set_keep is unchanged, so a direction pipe has a mask only on grids the masked scan accepts
 * too; on a grid that only mtgpu_dir_preview accepts, mtgpu_pipe_set_keep fails as before and the pipe runs unmasked
 * direction.  mtgpu_pipe_set_keep and mtgpu_pipe_set_dir commute.
 * Other modes: mtgpu_pipe_set_dir(enable != 0) on a pipe with blobs (mtgpu_pipe_set_blobs), compensation
 * (mtgpu_pipe_set_gmc) or the compensated blob scan (mtgpu_pipe_set_gmc_blobs) on, and each of those three setters
 * turning its mode on on a pipe with direction on, are MT_ERR_UNSUPPORTED ("not together yet", the other setter named),
 * and nothing changes.  Turning any mode off is always accepted.
 * With mtgpu_profile_enable on, a direction submit records one event triple, as a plain one.
 */
int mtgpu_pipe_set_dir(mtgpu_pipe *pipe, int enable, int32_t allow, int report);

/*
 * 1: the pipe's submits run the direction scan, and *allow / *report (each may be NULL) receive the setting; 0: they do
 * not, nothing is written; -1: pipe is NULL.
 */
int mtgpu_pipe_dir(const mtgpu_pipe *pipe, int32_t *allow /* may be NULL */, int *report /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_PIPE_DIR_H */
