/*
 * mtgpu_gmc_blobs.h — the compensated blob scan: motion blobs on the residuals of each frame's dominant vector.  Part of
 * the C ABI of mtgpu.h, which includes this header (include either one).  Same conventions: MT_* status codes, arguments
 * validated before anything is launched, the `*_device` entry point takes device pointers and is asynchronous on
 * `stream`, the other takes host pointers and is synchronous; NO CPU fallback; no environment variables.
 *
 * Compensation (mtgpu_gmc.h) removes the camera's own motion: a pole in wind or a PTZ tour no longer keeps every frame.
 * Blobs (mtgpu_blobs.h) ask for ONE object of N cells rather than N cells anywhere: rain, foliage and compression noise
 * no longer add up to an "object".  A shaking camera in the rain needs both.  What compensation leaves behind is
 * scattered residual noise — on that, CLUSTERS_NEEDED has exactly the weakness blobs were added to remove — and an
 * uncompensated blob scan of such a stream is useless: the whole panned region is one blob.  The residual vote exists
 * only inside the compensated scan's kernel, so the pair cannot be had by chaining calls; this scan labels it there.
 *
 * Semantics (everything is integer and exact).  Let gw, gh, m = vertical_margin, shift = block_shift, thr, vn =
 * vectors_needed and cn = clusters_needed be the context's.  Per call: max_shift in [0, 127], min_share_q8 in [0, 256]
 * (mtgpu_gmc.h) and min_blob_cells (mtgpu_blobs.h).  A call may carry per-stream keep planes d_keep / d_stream_off /
 * n_streams exactly as mtgpu_scan_blobs_device takes them: the stream lookup is that of mtgpu_zones.h, and a frame at
 * or behind stream_off[n_streams] reads the no-blob answer.  Per frame with side data, with K the frame's stream's
 * plane or "no mask":
 *
 *  1. counted   a record is counted iff it passes the bounds test of src/motion_scanner.cpp:262 (0 <= dst_x >> shift <
 *               gw and m <= dst_y >> shift < gh - m) and, under a mask, the keep bit of its destination cell is set.
 *               This is the masked estimate of mtgpu_pipe_gmc.h, for the reason given there: an overlay must neither
 *               vote in the estimate nor become motion after it.
 *  2. bins, mode, support   steps 2-4 of mtgpu_gmc.h, unchanged, over the counted records: (gx, gy) and the fields of
 *               mt_gmc_info.
 *  3. vote      step 5 of mtgpu_gmc.h: EVERY record inside the bounds votes its residual (rx, ry) = (dst - src) -
 *               (gx, gy) into its destination cell iff rx^2 + ry^2 >= thr, squares in 64 bits.  A cell is active iff
 *               votes >= vn and, under a mask on an analysed row, its keep bit is set: the plane of mtgpu_zones.h —
 *               halo rows are unmasked, and vn == 0 behaves as there.
 *  4. centres, blobs   C(f) and its 4-connected components exactly as mtgpu_blobs.h defines them on that plane;
 *               centres, blobs, largest, box and the tie rule (among blobs of equal maximal size the one that contains
 *               the smallest y * gw + x) are the same.
 *  5. flags     centres >= max(1, cn) AND largest >= max(1, min_blob_cells).
 *
 * Outputs, per frame f (each may be NULL, not all six):
 *   flags[f] uint8, centres[f], blobs[f], largest[f] uint32, box[f] mt_blob_box   as mtgpu_blobs.h
 *   info[f]  mt_gmc_info   the applied vector, the modes, n_in (the COUNTED records) and the modes' counts
 * A NULL output is never touched.  Every element of a non-NULL output is written, and exactly n_frames of them.  A frame
 * without side data (has_sd == NULL: the frame owns no record), or under a mask a frame at or behind
 * stream_off[n_streams], reads 0 everywhere, an all-0xFFFF box and an all-zero info.
 *
 * Consequences.
 *  A. max_shift == 0 equals mtgpu_scan_blobs_device with the same mask and min_blob_cells, bit for bit on all five blob
 *     outputs.  The same holds for any frame whose gx == gy == 0.
 *  B. Without a mask, centres and info equal mtgpu_scan_gmc_device's bit for bit.  With min_blob_cells <= 1, flags do
 *     too.
 *  C. A frame's five blob outputs equal mtgpu_scan_blobs_device's, with the same plane, on the frame with (gx, gy) added
 *     to every record's src, wherever that stays inside int16.
 *  D. With one stream and one plane, centres and (gx, gy) equal the compensated pipe's under that plane
 *     (mtgpu_pipe_gmc.h).
 *  E. For a level L >= max(1, cn): `largest`, handed to the unchanged mtgpu_sweep_streams_device as its d_centres with
 *     levels = {L, ...}, gives the segments of `flags` at min_blob_cells = L, bit for bit.
 *
 * The decode path: mtgpu_pipe_gmc_blobs.h carries this scan through the pipe as a mode of its own
 * (mtgpu_pipe_set_gmc_blobs), the C++ host layer and mtgpu_scan_file (--gmc-blobs); mtgpu_pipe_set_gmc and
 * mtgpu_pipe_set_blobs, set one after the other, still refuse the pair.  Out of scope: the row-banded grids (960x540, 32767-wide) are
 * MT_ERR_UNSUPPORTED with the grid named, as for both parents.
 *
 * Kernel (csrc/gmc_blobs_kernels.hip): one workgroup per frame with side data; the keep rows are staged in LDS, a first
 * pass over the frame's records fills the two histograms, one wave picks the modes, a second pass votes the residuals,
 * and the centre plane is labelled by union-find over the dead vote tile, as the blob scan does.  A frame without a
 * centre ends after the centre test.  The LDS size is the blob scan's plus the histograms' and depends on the grid
 * alone.
 */
#ifndef MTGPU_GMC_BLOBS_H
#define MTGPU_GMC_BLOBS_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mt_gmc_info (mtgpu_gmc.h) and mt_blob_box (mtgpu_blobs.h), by their struct tags: whichever of the three headers is
 * included first, mtgpu.h reaches this one before that header's own body, so the prototypes below cannot rely on the
 * typedefs. */
struct mt_gmc_info;
struct mt_blob_box;

/* How the compensated blob scan runs on a grid (src/motion_scanner.cpp:237-238: the analysed rows size the tile). */
typedef struct mtgpu_gmc_blobs_plan {
  int32_t lds_bytes;              /* dynamic LDS per workgroup                           */
  int32_t workgroup;              /* lanes                                               */
  int32_t keep_words_per_row;     /* W = (grid_w + 63) / 64                              */
  int32_t keep_words_per_stream;  /* grid_h * W: uint64 words of one stream's keep plane */
  int32_t hist_bins;              /* bins reserved per axis (max_shift 127 fits)         */
  int32_t info_bytes;             /* sizeof(mt_gmc_info)                                 */
} mtgpu_gmc_blobs_plan;

/*
 * The plan mtgpu_scan_gmc_blobs_device would pick for these parameters (the grid and the vertical margin of
 * src/motion_scanner.cpp:237-238 are all that matter) on a device with `lds_bytes_per_workgroup` of LDS per workgroup
 * (MI355X: 163840), and the sizes of a keep mask.  Pure host arithmetic: no HIP call, works without a device.
 * MT_ERR_INVALID: NULL / invalid parameters, LDS size below 1024; MT_ERR_UNSUPPORTED (the grid is named): the layout
 * does not fit.  out->lds_bytes <= lds_bytes_per_workgroup.
 */
int mtgpu_gmc_blobs_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, mtgpu_gmc_blobs_plan *out);

/*
 * The compensated blob scan of a device-resident batch; asynchronous on `stream`.  d_rec / rec_bytes / n_records /
 * d_frame_off / d_has_sd / n_frames as for mtgpu_scan_centres_device (rec_bytes 40 = mt_mv, 8 = mt_mv_compact, 8-byte
 * aligned); d_stream_off / n_streams / d_keep / min_blob_cells as for mtgpu_scan_blobs_device; max_shift / min_share_q8
 * as for mtgpu_scan_gmc_device.
 *   d_flags n_frames uint8; d_centres, d_blobs, d_largest n_frames uint32 each; d_box n_frames mt_blob_box; d_info
 *   n_frames mt_gmc_info; each or NULL
 * All six outputs NULL is MT_ERR_INVALID; a NULL output is never touched.  n_frames == 0: MT_OK, nothing is written.
 * MT_ERR_INVALID (the argument is named in mtgpu_last_error) for rec_bytes outside {8, 40}, max_shift outside [0, 127],
 * min_share_q8 outside [0, 256], a misaligned pointer, NULL d_frame_off, d_keep given with d_stream_off == NULL or
 * n_streams == 0, d_keep == NULL with d_stream_off given or n_streams != 0, and an output or d_keep that is not memory
 * of the context's device.  MT_ERR_UNSUPPORTED (the grid is named) as above.  Nothing is launched and no output byte is
 * touched when the call fails this way.  Launch scratch (32 bytes per frame) comes from the context's ring; with
 * mtgpu_profile_enable on, the call records the same event triple as a scan launch.
 */
int mtgpu_scan_gmc_blobs_device(mtgpu_ctx *ctx, const void *d_rec, int rec_bytes, uint64_t n_records,
                                const uint64_t *d_frame_off, const uint8_t *d_has_sd /* may be NULL */, uint32_t n_frames,
                                const uint64_t *d_stream_off /* NULL iff d_keep is NULL */, uint32_t n_streams,
                                const uint64_t *d_keep /* NULL: no mask */, int32_t max_shift, int32_t min_share_q8,
                                int32_t min_blob_cells, uint8_t *d_flags, uint32_t *d_centres, uint32_t *d_blobs,
                                uint32_t *d_largest, struct mt_blob_box *d_box, struct mt_gmc_info *d_info, void *stream);

/*
 * The same for a batch in HOST memory: copies the records the offsets span, the offsets, has_sd, stream_off and keep to
 * the device, runs the call above, copies the outputs back; synchronous.  mv / frame_off / has_sd / n_frames as for
 * mtgpu_scan_frames_centres; stream_off: n_streams + 1 entries and keep: n_streams * gh * W uint64, or both NULL with
 * n_streams 0.  MT_ERR_INVALID also for decreasing frame_off or stream_off and for stream_off[n_streams] != n_frames.
 */
int mtgpu_scan_frames_gmc_blobs(mtgpu_ctx *ctx, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd,
                                uint32_t n_frames, const uint64_t *stream_off, uint32_t n_streams, const uint64_t *keep,
                                int32_t max_shift, int32_t min_share_q8, int32_t min_blob_cells, uint8_t *flags,
                                uint32_t *centres, uint32_t *blobs, uint32_t *largest, struct mt_blob_box *box,
                                struct mt_gmc_info *info);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_GMC_BLOBS_H */
