/*
 * mtgpu_pipe_boxes.h — the largest blob's box on the decode path: a pipe (mtgpu.h, "Host dispatcher") whose batches
 * also carry, per frame, the mt_blob_box of mtgpu_blobs.h.  Part of the C ABI of mtgpu.h, which includes this header
 * (include either one).  Same conventions: MT_* status codes, arguments validated before anything is launched, NO CPU
 * fallback, no environment variables.
 *
 * Why: temporal persistence (mtgpu_persist.h) links a run of motion frames only while the largest blob stays within
 * `reach` cells of where it was — that is what removes rain that passes the blob rule somewhere else in every frame.
 * A run crosses batch and chunk borders, so the rule is applied ONCE per recording, on the flags and boxes pooled from
 * every batch and sorted by pts (mtgpu_persist_flags); no scan state is carried from one submit to the next.  What the
 * decode path lacked was the box: the pipe forms of the two blob kernels dropped it.
 *
 * Layout: MT_LAYOUT_BOXES (8), OR-ed into any other layout of mtgpu_pipe_create_layout.  A boxed pipe's staging block
 * gets one more DEVICE-written array behind the last one it has: (max_frames + 1) x sizeof(mt_blob_box) bytes on
 * 128-byte lines of its own, padded to 128 — no line holds both host-stored and device-stored bytes.  Without
 * MT_LAYOUT_ZERO_COPY the device mirror grows alike and a boxed submit in a blob mode queues one more D2H copy of
 * n_frames x 8 bytes.  A pipe without the flag allocates what it allocated before, byte for byte.
 * mtgpu_pipe_stats.layout reports the flag.
 *
 * Who writes it: a submit in the blob mode (mtgpu_pipe_set_blobs) or the compensated blob mode
 * (mtgpu_pipe_set_gmc_blobs).  In the plain, masked and compensated (mtgpu_pipe_set_gmc) modes a boxed pipe launches
 * exactly what an unboxed one launches, and mtgpu_batch_boxes refuses the batch.  The batch remembers at submit whether
 * its kernel wrote boxes.
 *
 * Contract.  box[f] is specified WHERE flags[f] != 0.  There it is exactly the `box` that mtgpu_scan_blobs_device (or
 * mtgpu_scan_gmc_blobs_device) returns for the same frame under the same settings and keep mask: the same largest blob,
 * the same tie rule (among blobs of equal maximal size the one that holds the smallest y * grid_w + x), rows offset by
 * the analysed band's first row.  Where flags[f] == 0 the element is UNSPECIFIED, and in a reused pinned block it may
 * hold an earlier batch's value: the planning kernel answers frames without side data and knows nothing of boxes, the
 * kernel's no-centre exit does not pay a third system-scope store per quiet frame, and persistence reads `box` only at
 * frames with a flag.  A caller that wants a value everywhere writes the all-0xFFFF "no blob" box where the flag is 0
 * (ScanPipe.drain_boxes and the C++ host layer do).
 *
 * Kernels (csrc/blobs_kernels.hip, csrc/gmc_blobs_kernels.hip, the boxed pipe forms): on the final exit lane 0 stores
 * the four uint16 as ONE 8-byte store, at system scope where the flags are (a zero-copy batch's pinned block).  The blob
 * kernel's box pass ran already; the compensated kernel's boxed form gains that pass and its barrier.  No additional
 * LDS.  A boxed submit stays planning + one kernel + one event, takes nothing from the context's scratch ring, and
 * records one profile triple.
 *
 * Out of scope: boxes for frames without a flag; `blobs` or mt_gmc_info through the pipe.
 */
#ifndef MTGPU_PIPE_BOXES_H
#define MTGPU_PIPE_BOXES_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* OR-ed into any layout of mtgpu_pipe_create_layout: every batch also carries the largest blob's box of every frame
 * with a flag, read with mtgpu_batch_boxes.  mtgpu_pipe_create does not set it. */
#define MT_LAYOUT_BOXES 8

/* mt_blob_box (mtgpu_blobs.h), by its struct tag: whichever header is included first, mtgpu.h reaches this one before
 * or after that header's own body, so the prototype below cannot rely on the typedef. */
struct mt_blob_box;

/*
 * The boxes of a collected batch, frame by frame next to the flags mtgpu_pipe_collect exposed: valid between
 * mtgpu_pipe_collect and mtgpu_pipe_release; 8-byte aligned.  See "Contract" above: specified where flags[f] != 0.
 * MT_ERR_INVALID, the reason named in mtgpu_last_error, and *box = NULL (where box is not NULL) for:
 *   a NULL argument;
 *   a batch of a pipe created without MT_LAYOUT_BOXES;
 *   a batch that is not collected (being filled, in flight, released);
 *   a batch submitted while the pipe ran neither the blob scan (mtgpu_pipe_set_blobs) nor the compensated blob scan
 *   (mtgpu_pipe_set_gmc_blobs).
 */
int mtgpu_batch_boxes(const mtgpu_batch *batch, const struct mt_blob_box **box);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_PIPE_BOXES_H */
