/*
 * mtgpu_zones.h — ignore zones: the centre scan with a per-stream keep mask over the grid cells.  Part of the C ABI of
 * mtgpu.h, which includes this header (include either one).  Same conventions: MT_* status codes, arguments validated
 * before anything is launched, the `*_device` entry point takes device pointers and is asynchronous on `stream`, the
 * other takes host pointers and is synchronous; NO CPU fallback; no environment variables.
 *
 * The reference can mask full-width strips at the top and bottom only (VERTICAL_MASK, src/motion_scanner.cpp:237-238,
 * 262).  A keep mask removes single cells: a burnt-in clock, a road at one side, a neighbour's window.
 *
 * Semantics.  Let gw, gh, m = vertical_margin and vn = vectors_needed be the context's (mtgpu_params_from_config).
 * Stream s owns frames [stream_off[s], stream_off[s + 1]), as in mtgpu_activity_map_device.
 *
 *   keep   uint64 keep[n_streams][gh][W], W = (gw + 63) / 64: cell (x, y) of stream s is bit x & 63 of word x >> 6 of
 *          row y.  Bit set: the cell is analysed; bit clear: the cell is ignored.  Bits at x >= gw have no effect.
 *          Bits of rows outside the analysed range [m, gh - m) have no effect: those rows behave exactly as they do
 *          in the scan, also as neighbour rows when vn == 0.
 *   rule   on the analysed rows, active(x, y) = votes(x, y) >= vn AND keep(x, y)  (:282 with one more term).  An
 *          ignored cell is never a centre and never counts as somebody's neighbour.  Everything else is :277-292
 *          without the early return, exactly as mtgpu_scan_centres_device computes it.
 *
 * Consequences.
 *  - With an all-ones mask the result equals mtgpu_scan_centres_device bit for bit, for every vn, 0 included.
 *  - vn >= 1: the result equals the plain scan of the same frames with every record removed whose destination cell
 *    (dst_x >> shift, dst_y >> shift) is ignored, has_sd passed explicitly and unchanged.
 *  - vn >= 1: a context with margin 0 and a mask that clears rows [0, m) and [gh - m, gh) equals a context with
 *    margin m and no mask.
 *  - vn == 0: every kept analysed cell is active and an ignored cell is inactive.  This is deliberately NOT record
 *    removal, under which a mask would do nothing.  The margin equivalence does NOT hold for vn == 0: the reference
 *    treats margin rows as active neighbours (:282 never looks at them), a cleared mask row is inactive.
 *
 * Outputs, per frame f:
 *   centres[f]      the centre count under the mask
 *   flags[f]        centres[f] >= max(1, clusters_needed)  (:288)
 *   centres_all[f]  the same frame's count WITHOUT the mask, from the same votes (no second read of the records): what
 *                   the zones removed is centres_all[f] - centres[f].  Equals mtgpu_scan_centres_device exactly.
 * A frame without side data (the scan's rule, :219-221; has_sd == NULL: the frame owns no record) reads 0 in every
 * output.
 *
 * Kernel (csrc/zones_kernels.hip): one workgroup per frame with side data; one tile of 32-bit vote counters in LDS;
 * the stream's keep words staged in LDS once per workgroup and ANDed in when a row's 64-bit active mask is formed —
 * one AND per 64 cells, nothing per record.  A grid for which one tile and the mask planes do not fit (960x540 cells,
 * 32767-wide grids: the grids the plain scan cuts into row bands, the class mtgpu_scan_sweep_device and
 * mtgpu_activity_map_device reject) is MT_ERR_UNSUPPORTED.
 */
#ifndef MTGPU_ZONES_H
#define MTGPU_ZONES_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How the masked scan runs on a grid (src/motion_scanner.cpp:237-238: the analysed rows size the tile). */
typedef struct mtgpu_zones_plan {
  int32_t lds_bytes;              /* dynamic LDS per workgroup                         */
  int32_t workgroup;              /* lanes                                             */
  int32_t keep_words_per_row;     /* W = (grid_w + 63) / 64                            */
  int32_t keep_words_per_stream;  /* grid_h * W: uint64 words of one stream's keep plane */
} mtgpu_zones_plan;

/*
 * The plan mtgpu_scan_zones_device would pick for these parameters (the grid and the vertical margin of
 * src/motion_scanner.cpp:237-238 are all that matter) on a device with `lds_bytes_per_workgroup` of LDS per workgroup
 * (MI355X: 163840), and the sizes of a keep mask.  Pure host arithmetic: no HIP call, works without a device.
 * MT_ERR_INVALID: NULL / invalid parameters, LDS size below 1024; MT_ERR_UNSUPPORTED (the grid is named): the tile and
 * the mask planes do not fit.  out->lds_bytes <= lds_bytes_per_workgroup.
 */
int mtgpu_zones_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, mtgpu_zones_plan *out);

/*
 * The masked centre scan (src/motion_scanner.cpp:242-292 per frame, :282 ANDed with the stream's keep bit) of a
 * device-resident batch; asynchronous on `stream`.  d_rec / rec_bytes / n_records / d_frame_off / d_has_sd / n_frames
 * as for mtgpu_scan_centres_device (rec_bytes 40 = mt_mv, 8 = mt_mv_compact, 8-byte aligned).
 *   d_stream_off  n_streams + 1 uint64 frame offsets (device), non-decreasing.  A frame at or past
 *                 d_stream_off[n_streams] belongs to no stream and reads 0 in every output.
 *   d_keep        n_streams * gh * W uint64 (device), see above
 *   d_flags       n_frames uint8, or NULL;   d_centres, d_centres_all   n_frames uint32 each, or NULL
 * Any one or two of the three outputs may be NULL (never touched then); all three NULL is MT_ERR_INVALID.  Every
 * element of every non-NULL output is written, and exactly n_frames of them.  n_frames == 0: MT_OK, nothing is
 * written.  MT_ERR_INVALID (the argument is named in mtgpu_last_error) for rec_bytes outside {8, 40}, a misaligned
 * pointer, NULL d_frame_off / d_stream_off / d_keep, n_streams == 0 with n_frames > 0, and an output or d_keep that is
 * not memory of the context's device.  MT_ERR_UNSUPPORTED (the grid is named) as above.  Nothing is launched and no
 * output byte is touched when the call fails this way.  Launch scratch (32 bytes per frame) comes from the context's
 * ring; with mtgpu_profile_enable on, the call records the same event triple as a scan launch.
 */
int mtgpu_scan_zones_device(mtgpu_ctx *ctx, const void *d_rec, int rec_bytes, uint64_t n_records,
                            const uint64_t *d_frame_off, const uint8_t *d_has_sd /* may be NULL */, uint32_t n_frames,
                            const uint64_t *d_stream_off, uint32_t n_streams, const uint64_t *d_keep,
                            uint8_t *d_flags, uint32_t *d_centres, uint32_t *d_centres_all, void *stream);

/*
 * The same for a batch in HOST memory (src/motion_scanner.cpp:217-295 for every frame, :282 ANDed with the keep bit):
 * copies the records the offsets span, the offsets, has_sd, stream_off and keep to the device, runs the call above,
 * copies the outputs back; synchronous.  mv / frame_off / has_sd / n_frames as for mtgpu_scan_frames_centres;
 * stream_off: n_streams + 1 entries; keep: n_streams * gh * W uint64; flags: n_frames uint8 or NULL; centres,
 * centres_all: n_frames uint32 or NULL.  MT_ERR_INVALID also for decreasing frame_off or stream_off and for
 * stream_off[n_streams] != n_frames.
 */
int mtgpu_scan_frames_zones(mtgpu_ctx *ctx, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd,
                            uint32_t n_frames, const uint64_t *stream_off, uint32_t n_streams, const uint64_t *keep,
                            uint8_t *flags, uint32_t *centres, uint32_t *centres_all);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_ZONES_H */
