/*
 * mtgpu_blobs.h — motion blobs: the connected components of a frame's centre cells.  Part of the C ABI of mtgpu.h,
 * which includes this header (include either one).  Same conventions: MT_* status codes, arguments validated before
 * anything is launched, the `*_device` entry point takes device pointers and is asynchronous on `stream`, the other
 * takes host pointers and is synchronous; NO CPU fallback; no environment variables.
 *
 * The reference counts a "cluster" per cell: an active cell with an active 4-neighbour (src/motion_scanner.cpp:272-294).
 * CLUSTERS_NEEDED = 8 therefore cannot tell one object of eight cells from four unrelated pairs of rain, foliage or
 * compression noise spread over the picture.  A blob scan adds the setting every trimmer user expects — a minimum
 * object size — and says where the largest object of a frame is.
 *
 * Semantics.  Let gw, gh, m = vertical_margin, vn = vectors_needed and clusters_needed be the context's.  The active
 * plane A of frame f is
 *   d_keep == NULL   what mtgpu_scan_centres_device uses;
 *   d_keep given     what mtgpu_scan_zones_device uses with that keep mask: the stream lookup, rows outside the analysed
 *                    range, vn == 0 and the "behind the last stream" rule are those of mtgpu_zones.h.
 * C(f), the centre cells, are exactly the cells centres[f] counts (:277-292): active, y in [m, gh - m), x in [1, gw - 2],
 * with an active 4-neighbour in A.
 * A BLOB is a 4-connected component of C(f): two centres belong together iff a path of horizontally or vertically
 * adjacent CENTRES joins them.  Blobs are components of centre cells, not of active cells.  Three kinds of active cell
 * are no centres and join nothing: cells in column 0 or column gw - 1, cells in a halo row (outside [m, gh - m)), and
 * active cells without an active neighbour.
 *
 * Outputs, per frame f (each may be NULL, at least one must not be):
 *   centres[f]   uint32  |C(f)|: mtgpu_scan_centres_device's count without a mask, mtgpu_scan_zones_device's `centres`
 *                        with one, bit for bit
 *   blobs[f]     uint32  the number of blobs
 *   largest[f]   uint32  the cell count of the largest blob; 0 if there is none
 *   box[f]       mt_blob_box  the inclusive cell bounds of the largest blob; among blobs of equal maximal size the one
 *                        that contains the smallest y * gw + x; all four fields 0xFFFF when there is no blob
 *   flags[f]     uint8   centres[f] >= max(1, clusters_needed) AND largest[f] >= max(1, min_blob_cells)  (:288 with
 *                        one more term)
 * A frame without side data (the scan's rule, :219-221; has_sd == NULL: the frame owns no record) reads 0 in every
 * output and an all-0xFFFF box; so does, under a mask, a frame at or past stream_off[n_streams].  Every element of
 * every non-NULL output is written.
 *
 * Consequences.
 *  - min_blob_cells <= 1: flags equals the flags of mtgpu_scan_centres_device — under a mask, of
 *    mtgpu_scan_zones_device — bit for bit.
 *  - blobs == 0  <=>  centres == 0  <=>  largest == 0.
 *  - largest <= centres.
 *  - blobs * largest >= centres.
 *  - For a level L >= max(1, clusters_needed): `largest`, handed to the unchanged mtgpu_sweep_streams_device as its
 *    d_centres with levels = {L, ...}, gives the segments of `flags` at min_blob_cells = L, bit for bit (largest >= L
 *    implies centres >= L >= clusters_needed).  One scan answers every MIN_BLOB_CELLS.
 *
 * Kernel (csrc/blobs_kernels.hip): one workgroup per frame with side data, the layout of the masked scan without its
 * unmasked plane; a frame without a centre ends after the centre test; otherwise the centre plane is labelled in LDS
 * by union-find over the dead vote tile.  A grid for which the tile, the keep rows and the mask plane do not fit
 * (960x540 cells, 32767-wide grids: the grids the plain scan cuts into row bands) is MT_ERR_UNSUPPORTED.
 *
 * Out of scope: there is no pipe form (mtgpu_pipe_*), no mtgpu_scan_file option and no decode-path scanner for blobs;
 * a blob scan is a call on a batch.  (That holds for the entry points of THIS header.  The decode path has its own:
 * mtgpu_pipe_blobs.h puts the flag rule and one of the two counts into a pipe.)  No compensation either: blobs on the
 * residuals of each frame's dominant vector are the resident scan of mtgpu_gmc_blobs.h; the pipe still refuses the pair.
 */
#ifndef MTGPU_BLOBS_H
#define MTGPU_BLOBS_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Inclusive cell bounds of a frame's largest blob (columns x0 .. x1, grid rows y0 .. y1); all 0xFFFF: no blob. */
typedef struct mt_blob_box {
  uint16_t x0, y0, x1, y1;
} mt_blob_box;

/* How the blob scan runs on a grid (src/motion_scanner.cpp:237-238: the analysed rows size the tile). */
typedef struct mtgpu_blobs_plan {
  int32_t lds_bytes;              /* dynamic LDS per workgroup                         */
  int32_t workgroup;              /* lanes                                             */
  int32_t keep_words_per_row;     /* W = (grid_w + 63) / 64                            */
  int32_t keep_words_per_stream;  /* grid_h * W: uint64 words of one stream's keep plane */
} mtgpu_blobs_plan;

/*
 * The plan mtgpu_scan_blobs_device would pick for these parameters (the grid and the vertical margin of
 * src/motion_scanner.cpp:237-238 are all that matter) on a device with `lds_bytes_per_workgroup` of LDS per workgroup
 * (MI355X: 163840), and the sizes of a keep mask.  Pure host arithmetic: no HIP call, works without a device.
 * MT_ERR_INVALID: NULL / invalid parameters, LDS size below 1024; MT_ERR_UNSUPPORTED (the grid is named): the layout
 * does not fit.  out->lds_bytes <= lds_bytes_per_workgroup.
 */
int mtgpu_blobs_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, mtgpu_blobs_plan *out);

/*
 * The blob scan (src/motion_scanner.cpp:272-294 per frame — :282 ANDed with the stream's keep bit where a mask is
 * given — then the components of the centres) of a device-resident batch; asynchronous on `stream`.  d_rec / rec_bytes
 * / n_records / d_frame_off / d_has_sd / n_frames as for mtgpu_scan_centres_device (rec_bytes 40 = mt_mv, 8 =
 * mt_mv_compact, 8-byte aligned).
 *   d_keep          n_streams * gh * W uint64 (device) as in mtgpu_zones.h, or NULL: no mask
 *   d_stream_off    n_streams + 1 uint64 frame offsets (device), non-decreasing; NULL iff d_keep is NULL
 *   n_streams       0 iff d_keep is NULL
 *   min_blob_cells  the least cell count of the largest blob for flags[f] = 1; values below 1 count as 1
 *   d_flags n_frames uint8; d_centres, d_blobs, d_largest n_frames uint32 each; d_box n_frames mt_blob_box; each or NULL
 * All five outputs NULL is MT_ERR_INVALID; a NULL output is never touched.  n_frames == 0: MT_OK, nothing is written.
 * MT_ERR_INVALID (the argument is named in mtgpu_last_error) for rec_bytes outside {8, 40}, a misaligned pointer, NULL
 * d_frame_off, d_keep given with d_stream_off == NULL or n_streams == 0, d_keep == NULL with d_stream_off given or
 * n_streams != 0, and an output or d_keep that is not memory of the context's device.  MT_ERR_UNSUPPORTED (the grid is
 * named) as above.  Nothing is launched and no output byte is touched when the call fails this way.  Launch scratch
 * (32 bytes per frame) comes from the context's ring; with mtgpu_profile_enable on, the call records the same event
 * triple as a scan launch.
 */
int mtgpu_scan_blobs_device(mtgpu_ctx *ctx, const void *d_rec, int rec_bytes, uint64_t n_records,
                            const uint64_t *d_frame_off, const uint8_t *d_has_sd /* may be NULL */, uint32_t n_frames,
                            const uint64_t *d_stream_off /* NULL iff d_keep is NULL */, uint32_t n_streams,
                            const uint64_t *d_keep /* NULL: no mask */, int32_t min_blob_cells, uint8_t *d_flags,
                            uint32_t *d_centres, uint32_t *d_blobs, uint32_t *d_largest, mt_blob_box *d_box, void *stream);

/*
 * The same for a batch in HOST memory (src/motion_scanner.cpp:217-295 for every frame, then the components of the
 * centres): copies the records the offsets span, the offsets, has_sd, stream_off and keep to the device, runs the call
 * above, copies the outputs back; synchronous.  mv / frame_off / has_sd / n_frames as for mtgpu_scan_frames_centres;
 * stream_off: n_streams + 1 entries and keep: n_streams * gh * W uint64, or both NULL with n_streams 0.  MT_ERR_INVALID
 * also for decreasing frame_off or stream_off and for stream_off[n_streams] != n_frames.
 */
int mtgpu_scan_frames_blobs(mtgpu_ctx *ctx, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd,
                            uint32_t n_frames, const uint64_t *stream_off, uint32_t n_streams, const uint64_t *keep,
                            int32_t min_blob_cells, uint8_t *flags, uint32_t *centres, uint32_t *blobs, uint32_t *largest,
                            mt_blob_box *box);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_BLOBS_H */
