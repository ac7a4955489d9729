/*
 * mtgpu_gmc.h — global-motion compensation: the centre scan against each frame's dominant vector.  Part of the C ABI of
 * mtgpu.h, which includes this header (include either one).  Same conventions: MT_* status codes, arguments validated
 * before anything is launched, the `*_device` entry point takes device pointers and is asynchronous on `stream`, the
 * other takes host pointers and is synchronous; NO CPU fallback; no environment variables.
 *
 * check_frame thresholds every vector's own magnitude (src/motion_scanner.cpp:246-251).  When the camera itself moves —
 * a pole in wind, a PTZ preset tour, a vibrating mount — nearly every record of the frame passes, every cell is active
 * and the frame is kept; no ignore zone and no blob size helps, the whole frame is one blob.  The compensated scan
 * estimates the frame's dominant vector from the records themselves, subtracts it, and runs the threshold, the vote and
 * the centres on the residuals.
 *
 * Semantics (everything is integer and exact).  Let gw, gh, m = vertical_margin, shift = block_shift, thr, vn =
 * vectors_needed and cn = clusters_needed be the context's (mtgpu_params_from_config), as in mtgpu_scan_centres_device.
 * Two parameters per call: max_shift in [0, 127] and min_share_q8 in [0, 256]; the Python layer and the command default
 * to MTGPU_GMC_DEFAULT_MAX_SHIFT = 16 and MTGPU_GMC_DEFAULT_MIN_SHARE_Q8 = 128.  Per frame with side data:
 *
 *  1. counted   a record is counted iff it passes the bounds test of :262, 0 <= dst_x >> shift < gw and
 *               m <= dst_y >> shift < gh - m: the test the vote uses.  n_in is their number.  Records in the masked
 *               margin rows (clock overlays) and outside the frame take no part in the estimate.
 *  2. bins      per axis, over the counted records: hx[v] = the number with dst_x - src_x == v for |v| <= max_shift,
 *               hy[v] likewise with dst_y - src_y.  A displacement beyond max_shift is in no bin of that axis; the
 *               record still counts in n_in.
 *  3. mode      per axis, walk the candidates in the order 0, -1, +1, -2, +2, ..., -max_shift, +max_shift; the first
 *               candidate whose count is maximal wins: (mode_x, n_x), (mode_y, n_y), n_* the winner's count.  With
 *               n_in == 0 both modes are 0.
 *  4. support   per axis independently: gx = mode_x if n_x * 256 >= min_share_q8 * n_in (in 64 bits), else 0; gy
 *               likewise.  The support test keeps a static camera's background of {-1, 0, +1} noise from being
 *               "compensated" by +-1 and pushed over a low threshold.
 *  5. vote      for each record rx = (dst_x - src_x) - gx, ry = (dst_y - src_y) - gy; the record is kept iff
 *               rx^2 + ry^2 >= thr, evaluated exactly (|rx| can reach 65 662: 64-bit products).  The cell is the
 *               destination cell, unchanged.  From here on everything is :262-292 without the early return, exactly as
 *               mtgpu_scan_centres_device computes it: votes, vn, the centres, vn == 0, out-of-grid neighbours inactive.
 *
 * Outputs, per frame f (each may be NULL, not all three):
 *   centres[f]   the centre count of the residual vote
 *   flags[f]     centres[f] >= max(1, cn)  (:288)
 *   info[f]      mt_gmc_info: the applied vector, the modes, n_in and the modes' counts
 * A frame without side data (the scan's rule, :219-221; has_sd == NULL: the frame owns no record) reads 0 in every
 * output, all fields of info included.
 *
 * Consequences.
 *  A. max_shift == 0 equals mtgpu_scan_centres_device bit for bit, for every vn.  The same holds for any frame whose
 *     gx == gy == 0.
 *  B. Translation invariance: if every record of a frame has (a, b) added to its src — dst, and so every cell,
 *     unchanged — the frame's gx, gy become gx - a, gy - b and centres does not change, provided both axes are supported
 *     before and after and the shifted modes stay within max_shift.
 *  C. A frame's centres equals the plain centre count of the same frame with (gx, gy) added to every record's src,
 *     wherever that stays inside int16.
 *  D. vn == 0: the result equals the plain centre scan (every cell of the grid is active whatever the votes are).
 *
 * Out of scope: keep masks; blobs; the pipe form and mtgpu_scan_file — of THESE entry points: the resident scan with
 * blobs and per-stream keep masks is mtgpu_gmc_blobs.h, and the decode path has its own two entry points, which honour
 * the pipe's keep mask in the estimate and in the vote (mtgpu_pipe_gmc.h) and still refuse blobs next to them; the
 * row-banded grids (960x540, 32767-wide), which are MT_ERR_UNSUPPORTED with the grid named, as for the zones and the
 * blobs; rotation or zoom models — this is a translation only; any use of neighbouring frames — frames stay independent.
 *
 * Kernel (csrc/gmc_kernels.hip): one workgroup per frame with side data; a first pass over the frame's records fills two
 * histograms in LDS, one wave picks the modes, a second pass over the same records votes the residuals into one tile of
 * 32-bit counters in LDS.  The LDS size depends on the grid alone (the histograms are sized for max_shift 127).
 */
#ifndef MTGPU_GMC_H
#define MTGPU_GMC_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTGPU_GMC_MAX_SHIFT 127
#define MTGPU_GMC_DEFAULT_MAX_SHIFT 16
#define MTGPU_GMC_DEFAULT_MIN_SHARE_Q8 128

/* What the estimate found for one frame; 20 bytes, 4-byte aligned. */
typedef struct mt_gmc_info {
  int16_t gx, gy;          /* the vector that was subtracted (0 on an axis without support)  */
  int16_t mode_x, mode_y;  /* the modes of the two axes                                      */
  uint32_t n_in;           /* counted records (:262)                                         */
  uint32_t n_x, n_y;       /* the modes' counts                                              */
} mt_gmc_info;

/* How the compensated scan runs on a grid (src/motion_scanner.cpp:237-238: the analysed rows size the tile). */
typedef struct mtgpu_gmc_plan {
  int32_t lds_bytes;       /* dynamic LDS per workgroup                     */
  int32_t workgroup;       /* lanes                                         */
  int32_t hist_bins;       /* bins reserved per axis (max_shift 127 fits)   */
  int32_t info_bytes;      /* sizeof(mt_gmc_info)                           */
} mtgpu_gmc_plan;

/*
 * The plan mtgpu_scan_gmc_device would pick for these parameters (the grid and the vertical margin of
 * src/motion_scanner.cpp:237-238 are all that matter) on a device with `lds_bytes_per_workgroup` of LDS per workgroup
 * (MI355X: 163840).  Pure host arithmetic: no HIP call, works without a device.  MT_ERR_INVALID: NULL / invalid
 * parameters, LDS size below 1024; MT_ERR_UNSUPPORTED (the grid is named): the tile, the mask plane and the histograms
 * do not fit.  out->lds_bytes <= lds_bytes_per_workgroup.
 */
int mtgpu_gmc_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, mtgpu_gmc_plan *out);

/*
 * The compensated centre scan (src/motion_scanner.cpp:242-292 per frame, :246-251 on the residuals of the frame's
 * dominant vector) of a device-resident batch; asynchronous on `stream`.  d_rec / rec_bytes / n_records / d_frame_off /
 * d_has_sd / n_frames as for mtgpu_scan_centres_device (rec_bytes 40 = mt_mv, 8 = mt_mv_compact, 8-byte aligned).
 *   d_flags    n_frames uint8, or NULL;   d_centres   n_frames uint32, or NULL;   d_info   n_frames mt_gmc_info, or NULL
 * Any one or two of the three outputs may be NULL (never touched then); all three NULL is MT_ERR_INVALID.  Every element
 * of every non-NULL output is written, and exactly n_frames of them.  n_frames == 0: MT_OK, nothing is written.
 * MT_ERR_INVALID (the argument is named in mtgpu_last_error) for max_shift outside [0, 127], min_share_q8 outside
 * [0, 256], rec_bytes outside {8, 40}, a misaligned pointer, NULL d_frame_off, and an output that is not memory of the
 * context's device.  MT_ERR_UNSUPPORTED (the grid is named) as above.  Nothing is launched and no output byte is touched
 * when the call fails this way.  Launch scratch (32 bytes per frame) comes from the context's ring; with
 * mtgpu_profile_enable on, the call records the same event triple as a scan launch.
 */
int mtgpu_scan_gmc_device(mtgpu_ctx *ctx, const void *d_rec, int rec_bytes, uint64_t n_records, const uint64_t *d_frame_off,
                          const uint8_t *d_has_sd /* may be NULL */, uint32_t n_frames, int32_t max_shift,
                          int32_t min_share_q8, uint8_t *d_flags, uint32_t *d_centres, mt_gmc_info *d_info, void *stream);

/*
 * The same for a batch in HOST memory (src/motion_scanner.cpp:217-295 for every frame, :246-251 on the residuals):
 * copies the records the offsets span, the offsets and has_sd to the device, runs the call above, copies the outputs
 * back; synchronous.  mv / frame_off / has_sd / n_frames as for mtgpu_scan_frames_centres; flags: n_frames uint8 or NULL;
 * centres: n_frames uint32 or NULL; info: n_frames mt_gmc_info or NULL.  MT_ERR_INVALID also for decreasing frame_off.
 */
int mtgpu_scan_frames_gmc(mtgpu_ctx *ctx, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd,
                          uint32_t n_frames, int32_t max_shift, int32_t min_share_q8, uint8_t *flags, uint32_t *centres,
                          mt_gmc_info *info);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_GMC_H */
