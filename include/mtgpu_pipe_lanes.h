/*
 * mtgpu_pipe_lanes.h — direction planes on the decode path: a pipe (mtgpu.h, "Host dispatcher") in which a record votes
 * only if the allow byte of its DESTINATION CELL has the bit of its sector (mtgpu_lanes.h), under the keep mask of
 * mtgpu_pipe_zones.h where the pipe carries one.  Part of the C ABI of mtgpu.h, which includes this header (include
 * either one).  Same conventions: MT_* status codes, arguments validated before anything is launched, NO CPU fallback,
 * no environment variables.
 *
 * mtgpu_scan_lanes_device and `python -m mvtrim_amd.lanes --learn --save-plane` draw a plane and study it on a batch
 * that is already resident.  These two entry points put the plane where a recording is actually trimmed: decoder ->
 * mtgpu_batch_add_frame -> mtgpu_pipe_submit -> flags -> merge.  mtgpu_pipe_set_dir has one byte for the whole picture
 * there, which cannot describe a two-way road, a gate beside a pavement or a conveyor across a hall (mtgpu_lanes.h).
 *
 * Why the keep mask belongs to it.  A lane that should not vote is handled by the plane, a burnt-in clock by the mask,
 * and real cameras have both (mtgpu_pipe_dir.h).  A plane byte of 0 is NOT a keep bit of 0: a record of a byte-0 cell
 * still counts in the rose and in the sector word, and a record without a sector still votes there.
 *
 * Semantics (integer, exact; mtgpu_pipe_dir.h with the byte read per cell).  A pipe in plane mode has ONE plane P (gh
 * rows of gw bytes, row-major: the byte of cell (x, y) is P[y * gw + x]; bit k: sector k of mtgpu_dir.h is allowed) and a
 * keep plane K (mtgpu_pipe_set_keep; gh rows of W = (gw + 63) / 64 words, bit x & 63 of word x >> 6 of row y) or none.
 * It treats every frame with side data as follows.
 *
 *  1. counts    a record COUNTS iff it passes the bounds test and the threshold of mtgpu_dir.h step 1 and, where the
 *               pipe has a keep plane, the keep bit of its destination cell is set.
 *  2. n[k]      the number of counting records of sector k, for every k, WHATEVER the plane says.  Records without a
 *               sector are in no n[k].
 *  3. vote      every record that passes step 1 WITHOUT the keep condition, and for which bit k of the plane byte of its
 *               destination cell is set (k: its sector), votes for its destination cell.  A record without a sector
 *               always votes.
 *  4. active    the active plane is the masked one of mtgpu_zones.h: on the analysed rows a cell is active iff it has
 *               vectors_needed votes AND its keep bit is set (vectors_needed == 0: iff its keep bit is set); rows
 *               outside the analysed range behave as in the scan.  Centres and flags are then those of
 *               mtgpu_scan_lanes_device, taken on that plane.  (An implementation may skip the vote of a record in a
 *               keep-0 cell: the cell is inactive whatever its votes, so the result is the same.)
 *  5. MT_PIPE_REPORT_CENTRES   mtgpu_batch_centres holds the centre count.
 *  6. MT_PIPE_REPORT_SECTORS   mtgpu_batch_centres holds one word, the frame's SECTOR WORD:
 *               bits 0 .. 7     the present byte: bit k is set iff n[k] >= 1
 *               bits 8 .. 10    k*, the smallest k whose n[k] is maximal; 0 when every n[k] is 0
 *               bits 11 .. 31   min(n[k*], 2^21 - 1)
 *               A frame without a counting moving record reads 0.  The flag is the same under either report.
 * A frame without side data reads flag 0 and word 0 (under either report): the planning kernel answers it, as in every
 * other pipe form.  A frame whose analysed range is empty reads flag 0 and word 0 too.
 *
 * Consequences (what the tests hold).
 *  P1. Without a keep plane, flags and centres equal mtgpu_scan_frames_lanes in its one-plane form (stream_off NULL) on
 *      the same frames, bit for bit, and the sector word equals the word derived from its rose.
 *  P2. An all-ones keep plane equals no keep plane.
 *  P3. A plane filled with one byte b equals the direction pipe (mtgpu_pipe_set_dir) with allow = b, under either report,
 *      with and without a keep plane.  So b = 0xFF with the centre report equals the pipe without the mode: the plain
 *      pipe without a mask, the masked pipe with one.
 *  P4. With a keep plane: the centres equal what the masked pipe (no plane) gives for the frames with every record
 *      removed whose sector its destination cell forbids; the sector word equals the word derived from the resident rose
 *      of the frames with the records of keep-0 cells removed.
 *  P5. The sector word does not depend on the plane.
 *  P6. Plane bits are monotone: a plane whose bits are a subset of another's gives centres <=, frame by frame (fewer
 *      votes, a subset of the active cells, and the centre rule has no inhibition).
 *
 * The staging block of a batch has the flag bytes and ONE count array (MT_LAYOUT_CENTRES).  So a plane pipe reports the
 * flags and one 32-bit word per frame, chosen by `report`, exactly as a direction pipe does.
 *
 * Out of scope: a full mt_dir_rose array through the pipe (a layout bit of its own, as MT_LAYOUT_BOXES was); per-stream
 * planes on a pipe (one pipe, one camera: give each camera its own pipe); a flow map on the decode path (planes are
 * learned on resident batches, mtgpu_flow_frames / `python -m mvtrim_amd.lanes --learn`); planes together with blobs,
 * compensation or the compensated blob scan — the setters refuse each other (MT_ERR_UNSUPPORTED, "not together yet");
 * the row-banded grids.
 *
 * Kernel (csrc/lanes_kernels.hip, lanes_pipe_kernel): the plane scan without its clear kernel — the planning kernel
 * answers the frames without side data — without the stream lookup and the rose array, and with system-scope result
 * stores where the batch's results live in pinned host memory (MT_LAYOUT_ZERO_COPY), on the one exit the kernel has.
 * Lane 0 builds the sector word from the eight rose words in LDS.  The plane's analysed rows are staged in LDS where they
 * fit next to the tile (mtgpu_lanes_preview's `staged`), and read from memory, one cached byte per counting record, where
 * they do not.  The keep plane takes no additional LDS: the keep words of the analysed rows wait in the mask rows they
 * are ANDed into, so the supported grids are exactly those of mtgpu_lanes_preview.  A submit stays planning + one kernel
 * + one event.  The work list lies in the batch's own block: a plane submit takes no launch scratch from the context's
 * ring.
 */
#ifndef MTGPU_PIPE_LANES_H
#define MTGPU_PIPE_LANES_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * A direction plane for the decode path: the pipe that stands for the check_frame call in the decode loop
 * (src/motion_scanner.cpp:375-383) runs the plane scan for every batch submitted from now on.
 *   plane != NULL   on.  plane: grid_h x grid_w bytes of host memory (the context's grid), copied before the call
 *                   returns; the pipe owns ONE device copy, allocated on first use, kept across off / on and freed by
 *                   mtgpu_pipe_destroy.  report: MT_PIPE_REPORT_CENTRES, or MT_PIPE_REPORT_SECTORS — mtgpu_batch_centres
 *                   then holds the sector word, the flag is unchanged — which needs a pipe with MT_LAYOUT_CENTRES.  Any
 *                   other value is MT_ERR_INVALID.
 *   plane == NULL   off: the pipe is bit for bit a pipe that never had a plane, plain or masked as before.  `report` is
 *                   ignored and reset.
 * May be called only while no batch of the pipe is being filled or in flight (states 1 and 2; batches that are
 * collected but not yet released do not matter): otherwise MT_ERR_BUSY, and nothing changes — the same rule as
 * mtgpu_pipe_set_keep.  MT_ERR_INVALID: pipe is NULL.  MT_ERR_UNSUPPORTED (the grid is named): a grid
 * mtgpu_lanes_preview rejects; the setting stays off and the pipe goes on scanning as before.  A failing call launches
 * nothing.
 * Keep mask: mtgpu_pipe_set_keep is unchanged, so a plane pipe has a mask only on grids the masked scan accepts too; on a
 * grid that only mtgpu_lanes_preview accepts, mtgpu_pipe_set_keep fails as before and the pipe runs the unmasked plane
 * scan.  mtgpu_pipe_set_keep and mtgpu_pipe_set_plane commute.
 * The scalar direction mode: a plane and mtgpu_pipe_set_dir's byte are one rule at two granularities.
 * mtgpu_pipe_set_plane(plane != NULL) on a pipe with mtgpu_pipe_set_dir on, and mtgpu_pipe_set_dir(enable != 0) on a
 * plane pipe, are MT_ERR_INVALID with the other setter named in parentheses, and nothing changes.  mtgpu_pipe_dir reads 0
 * on a plane pipe.
 * Other modes: mtgpu_pipe_set_plane(plane != NULL) on a pipe with blobs (mtgpu_pipe_set_blobs), compensation
 * (mtgpu_pipe_set_gmc) or the compensated blob scan (mtgpu_pipe_set_gmc_blobs) on, and each of those three setters
 * turning its mode on on a plane pipe, are MT_ERR_UNSUPPORTED ("not together yet", the other setter named), and nothing
 * changes.  Turning any mode off is always accepted.
 * With mtgpu_profile_enable on, a plane submit records one event triple, as a plain one.
 */
int mtgpu_pipe_set_plane(mtgpu_pipe *pipe, const uint8_t *plane /* gh x gw bytes, host; NULL: off */, int report);

/*
 * 1: the pipe's submits run the plane scan; plane (gh x gw bytes, or NULL) receives the bytes and *report (may be NULL)
 * the report; 0: they do not, nothing is written; -1: pipe is NULL.
 */
int mtgpu_pipe_plane(const mtgpu_pipe *pipe, uint8_t *plane /* gh x gw bytes or NULL */, int *report /* or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_PIPE_LANES_H */
