/*
 * mtgpu_motion.h — the reference's per-second "motion scalar" on the MI355X: part of the C ABI of mtgpu.h, which
 * includes this header (include either one).  Same conventions: MT_* status codes, `*_device` entry points take device
 * pointers (or driver-allocated pinned host memory through its device address) and are asynchronous on `stream`, the
 * other takes host pointers and is synchronous; NO CPU fallback (MT_ERR_DEVICE from mtgpu_create without a usable
 * device); no environment variables.  Nothing here depends on the context's scan parameters, only on its device.
 *
 * What is computed (tools/motion_scalar.cpp:61-84, BASELINE configuration 1), over 40-byte AVMotionVector records
 * (mt_mv; compact records do not carry the fields):
 *     for every record with motion_scale != 0                                   (:75-76)
 *         dx = double(motion_x) / motion_scale, dy = double(motion_y) / motion_scale      (:78-79)
 *         bin[floor(pts_seconds)] += sqrt(dx * dx + dy * dy) * w * h                       (:66, :81-82)
 * in fp64.  Every TERM has exactly the bits the reference's code computes (IEEE division and square root, the
 * reference's order of operations, no contraction).  The SUM of a frame is a fixed reduction tree, not the reference's
 * record-by-record order: the same call on the same buffers gives the same bits, and the value differs from the
 * sequential sum by rounding only — all terms are >= 0, so by at most (2n + 2) * 2^-53 relative for n addends.  A bin
 * then adds its frames' sums in ascending frame order, exactly.
 */
#ifndef MTGPU_MOTION_H
#define MTGPU_MOTION_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Per-frame motion scores of a device-resident batch: the inner loop of tools/motion_scalar.cpp:68-83 for every frame.
 *   d_mv         n_records * 40 bytes, 4-byte aligned (8-byte aligned batches stream whole 128-byte lines)
 *   d_frame_off  n_frames + 1 uint64 record offsets, non-decreasing; entries are clamped to n_records
 *   d_scores     n_frames doubles, 8-byte aligned: the frame's sum of sqrt(dx^2 + dy^2) * w * h over its records with
 *                motion_scale != 0; +0.0 for a frame without such records
 *   d_terms      n_frames uint32 or NULL: the number of those records (the tool creates a CSV row for a second exactly
 *                when such a record falls into it, :82; also the n of the error bound above).  A frame holds fewer
 *                than 2^32 records.
 * Outputs in pinned host memory are written with system-scope stores, one per frame, as mtgpu_scan_centres_device
 * writes its counts.  Launch scratch (32 bytes per frame) comes from the context's ring.  One workgroup per frame with
 * records: a launch of a few frames, or of very small frames, does not fill the chip.
 */
int mtgpu_motion_scores_device(mtgpu_ctx *ctx, const void *d_mv, uint64_t n_records, const uint64_t *d_frame_off,
                               uint32_t n_frames, double *d_scores, uint32_t *d_terms /* may be NULL */, void *stream);

/*
 * Per-second bins of S streams from per-frame scores: the accumulation of tools/motion_scalar.cpp:62-66 and :82.
 *   d_scores, d_pts   F doubles each (F = d_stream_off[n_streams]): the frames' scores and timestamps in seconds
 *   d_terms           F uint32 or NULL (then d_bin_terms must be NULL)
 *   d_stream_off      n_streams + 1 uint64 frame offsets: stream s owns frames [d_stream_off[s], d_stream_off[s + 1])
 *   d_acc             n_streams * n_sec doubles: d_acc[s * n_sec + b] = the scores of stream s's frames with
 *                     floor(pts) == b, added in ascending frame order starting from +0.0 — bit for bit a sequential sum
 *   d_bin_terms       n_streams * n_sec uint64 or NULL: the same sum over d_terms
 * A frame is skipped when its timestamp is negative (how the host layers encode the JSON null of :62-63), NaN, or
 * floor(pts) >= n_sec.  Every bin is written (+0.0 / 0 where no frame falls).  MT_ERR_INVALID when n_sec == 0.
 */
int mtgpu_motion_bins_device(mtgpu_ctx *ctx, const double *d_scores, const uint32_t *d_terms /* may be NULL */,
                             const double *d_pts, const uint64_t *d_stream_off, uint32_t n_streams, uint32_t n_sec,
                             double *d_acc, uint64_t *d_bin_terms /* may be NULL */, void *stream);

/*
 * The whole of tools/motion_scalar.cpp:61-84 for one stream in HOST memory: copies the records the offsets span, the
 * offsets and the timestamps to the device, runs the two steps above, copies the bins back; synchronous.
 *   mv          records; frame f owns [frame_off[f], frame_off[f + 1])        frame_off   n_frames + 1, non-decreasing
 *   pts         n_frames doubles, seconds (negative = null)                    acc         n_sec doubles
 *   bin_terms   n_sec uint64 or NULL: a second has a CSV row in the tool's output iff bin_terms[second] > 0
 * MT_ERR_INVALID for NULL required pointers, n_sec == 0 and decreasing offsets.
 */
int mtgpu_motion_scalar(mtgpu_ctx *ctx, const mt_mv *mv, const uint64_t *frame_off, const double *pts,
                        uint32_t n_frames, uint32_t n_sec, double *acc, uint64_t *bin_terms /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_MOTION_H */
