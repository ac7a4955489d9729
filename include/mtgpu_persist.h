/*
 * mtgpu_persist.h — temporal persistence: the run lengths of motion frames per stream.  Part of the C ABI of mtgpu.h,
 * which includes this header (include either one).  Same conventions: MT_* status codes, arguments validated before
 * anything is launched, the `*_device` entry point takes device pointers and is asynchronous on `stream`, the other
 * takes host pointers and is synchronous; NO CPU fallback; no environment variables.
 *
 * Every rule of the scans is a rule about ONE frame.  The reference pools the pts of every frame whose check_frame is
 * true (src/motion_scanner.cpp:382-383) and merges timestamps within MAX_GAP_SEC of each other (src/pipeline.cpp:
 * 328-344), so one isolated false frame — a headlight sweep, an insect on the lens — costs a segment of 2 x PADDING_SEC,
 * and one such frame every MAX_GAP_SEC keeps a whole recording.  This call asks "did it keep moving?": it groups a
 * stream's motion frames into runs and tells every frame how long its run is.
 *
 * Semantics (everything is integer and exact).  The input is a batch of n_frames frames in S = n_streams streams
 * (stream_off: S + 1 frame offsets, as in mtgpu_merge_streams_device).  Each frame has flags[f] from any scan of this
 * library; optional per-frame inputs are has_sd[f] and box[f] (mt_blob_box, mtgpu_blobs.h).
 *
 * Frame classes inside a stream:
 *   M   flags[f] != 0.
 *   T   (transparent) otherwise, has_sd != NULL && has_sd[f] == 0.  These are key frames: they were never analysed and
 *       must not break a run.  Without this rule every GOP ends every run.
 *   Q   otherwise: the frame was analysed and was quiet.
 *
 * For an M frame f:
 *   p(f)    the previous M frame of the same stream, or none.
 *   q(f)    the number of Q frames strictly between p(f) and f.
 *   brk(f)  1 iff p(f) is none, or q(f) > max_dropout, or box != NULL and linked(box[p(f)], box[f]) is false.
 * linked(A, B) is false if either box is the all-0xFFFF "no blob" box.  Otherwise it is true iff all four hold:
 *   B.x0 <= A.x1 + reach,  A.x0 <= B.x1 + reach,  B.y0 <= A.y1 + reach,  A.y0 <= B.y1 + reach
 * in arithmetic of at least 32 bits; reach is in [0, 65535] and is ignored when box is NULL.
 *
 * A run is an M frame with brk = 1 together with the M frames after it, up to the one before the next brk = 1.  Links
 * are between consecutive M frames only.
 *
 * Outputs, per frame (each may be NULL, not all three; every element of every non-NULL output is written):
 *   run[f]        uint32   M frame: the number of M frames in its run.  Q or T frame: 0.
 *   pos[f]        uint32   M frame: its 1-based ordinal inside the run, else 0.  pos == 1 marks a run's first frame; a
 *                          causal rule ("from the N-th frame on") is pos >= N.
 *   flags_out[f]  uint8    flags[f] != 0 && run[f] >= max(1, min_run), written as 0 / 1.
 * Frames outside [stream_off[0], stream_off[S]) read 0 in every output.
 *
 * Consequences.
 *  A. min_run <= 1: flags_out[f] = (flags[f] != 0) inside the streams.
 *  B. box == NULL and max_dropout = 0xFFFFFFFF: every M frame of a stream has run equal to the number of M frames of
 *     the stream.
 *  C. box == NULL, has_sd == NULL, max_dropout = 0: run is the length of the maximal block of consecutive non-zero
 *     flags.
 *  D. Inside a run, pos counts 1 .. run.  The sum of run over the frames with pos == 1 is the number of M frames.
 *  E. For a level L >= 1: `run`, handed to the unchanged mtgpu_sweep_streams_device as its d_centres with levels =
 *     {L, ...}, gives the segments of mtgpu_merge_streams_device on flags_out at min_run = L, bit for bit.  One pass
 *     answers every MIN_RUN.
 *  F. Raising max_dropout or reach never lowers any run[f].
 *  G. A stream's outputs equal those of a call on that stream alone.
 *
 * On the decode path (mtgpu_pipe_boxes.h; the C++ host layer; mtgpu_scan_file --min-run): a run crosses batch and chunk
 * boundaries, and the chunks of a recording are scanned in any order, so nothing is carried from one submit to the next —
 * the flags, has_sd and (from a pipe with MT_LAYOUT_BOXES) the boxes of every batch are pooled, sorted by pts, and THIS
 * call runs once per recording.
 *
 * Out of scope: the pipe's kernels carry no run state (see above: mtgpu_pipe_boxes.h is what the decode path adds); a
 * level sweep of another setting under persistence; run duration in seconds; filling the bridged Q frames (the merge's
 * MAX_GAP_SEC covers them); tracking more than the largest blob.
 *
 * Kernel (csrc/persist_kernels.hip): one workgroup per stream, as the merge launches; the workgroup walks the stream in
 * tiles of frames_per_tile frames, forwards for pos and backwards for run, with wave64 scans joined across the waves in
 * LDS and the state carried from tile to tile.  A long stream is NOT split over several workgroups: a call on one
 * stream runs on one compute unit.
 */
#ifndef MTGPU_PERSIST_H
#define MTGPU_PERSIST_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mt_blob_box (mtgpu_blobs.h), by its struct tag: whichever of the two headers is included first, mtgpu.h reaches this
 * one before or after that header's own body, so the prototypes below cannot rely on the typedef. */
struct mt_blob_box;

/* How the persistence pass runs. */
typedef struct mtgpu_persist_plan {
  int32_t workgroup;        /* lanes */
  int32_t frames_per_tile;  /* frames a workgroup takes per step */
} mtgpu_persist_plan;

/* The plan of mtgpu_persist_flags_device: workgroup is a multiple of 64, frames_per_tile a multiple of workgroup.  Pure
 * host, no device.  MT_ERR_INVALID: out is NULL. */
int mtgpu_persist_preview(mtgpu_persist_plan *out);

/*
 * The runs of a device-resident batch; asynchronous on `stream`.
 *   d_flags       n_frames uint8                            d_has_sd   n_frames uint8 or NULL
 *   d_box         n_frames mt_blob_box or NULL              d_stream_off   n_streams + 1 uint64, non-decreasing; entries
 *                                                           above n_frames are read as n_frames
 *   d_work        n_frames uint32: the caller's workspace, in the d_ts idiom of mtgpu_merge_streams_device.  Its
 *                 contents are unspecified afterwards.  The call allocates nothing and takes nothing from the
 *                 context's scratch ring.
 *   d_flags_out   n_frames uint8; d_run, d_pos n_frames uint32 each; each or NULL
 * MT_ERR_INVALID (the argument is named in mtgpu_last_error) for: all three outputs NULL; NULL d_flags, d_stream_off or
 * d_work with n_frames > 0; n_streams == 0 with n_frames > 0; reach > 65535; a misaligned pointer; an output or d_work
 * that is not memory of the context's device; an output or d_work whose byte range overlaps an input's or another
 * output's — there is NO in-place form: d_flags_out must not be d_flags.  n_frames == 0: MT_OK, and nothing is touched.
 * Nothing is launched and no byte is written when a call fails this way.  reach is ignored when d_box is NULL.
 */
int mtgpu_persist_flags_device(mtgpu_ctx *ctx, const uint8_t *d_flags, const uint8_t *d_has_sd /* may be NULL */,
                               const struct mt_blob_box *d_box /* may be NULL */, uint32_t n_frames,
                               const uint64_t *d_stream_off, uint32_t n_streams, uint32_t min_run, uint32_t max_dropout,
                               uint32_t reach, uint32_t *d_work /* n_frames words */, uint8_t *d_flags_out, uint32_t *d_run,
                               uint32_t *d_pos, void *stream);

/*
 * The same for a batch in HOST memory: copies the inputs to the device, runs the call above with a workspace of its own,
 * copies the outputs back; synchronous.  MT_ERR_INVALID also for decreasing stream_off and for stream_off[n_streams] >
 * n_frames.
 */
int mtgpu_persist_flags(mtgpu_ctx *ctx, const uint8_t *flags, const uint8_t *has_sd, const struct mt_blob_box *box,
                        uint32_t n_frames, const uint64_t *stream_off, uint32_t n_streams, uint32_t min_run,
                        uint32_t max_dropout, uint32_t reach, uint8_t *flags_out, uint32_t *run, uint32_t *pos);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_PERSIST_H */
