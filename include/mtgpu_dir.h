/*
 * mtgpu_dir.h — the direction filter: the centre scan in which a record votes only if the sector of its displacement is
 * allowed, and the per-frame motion rose.  Part of the C ABI of mtgpu.h, which includes this header (include either
 * one).  Same conventions: MT_* status codes, arguments validated before anything is launched, the `*_device` entry
 * point takes device pointers and is asynchronous on `stream`, the other takes host pointers and is synchronous; NO CPU
 * fallback; no environment variables.
 *
 * The reference squares dst - src (src/motion_scanner.cpp:246-251) and the sign is gone: it asks how much a block
 * moves, never which way.  A camera over a one-way street wants the walker against the traffic; a gate wants arrivals,
 * not departures; a conveyor moves all day in one direction across the middle of the picture, where a zone would blind
 * the camera.  The data is in every record: dst_x - src_x and dst_y - src_y.
 *
 * Semantics.  Everything is integer and exact.  Let gw, gh, m = vertical_margin, shift, thr, vn and cn be the
 * context's, as in mtgpu_scan_centres_device.  For a record, dx = dst_x - src_x and dy = dst_y - src_y, so |dx| and |dy|
 * are at most 65535; ax = |dx|, ay = |dy|.
 *
 * Sector of a record.  The picture's x grows to the right and y grows downwards; sectors are numbered clockwise on the
 * screen.
 *
 *     k      name      rule
 *     -      none      dx == 0 && dy == 0
 *     0      E         12 ay <= 5 ax, dx > 0
 *     4      W         12 ay <= 5 ax, dx < 0
 *     2      S         12 ax <= 5 ay, dy > 0
 *     6      N         12 ax <= 5 ay, dy < 0
 *     1 / 7  SE / NE   neither of the above, dx > 0, dy > 0 / dy < 0
 *     3 / 5  SW / NW   neither of the above, dx < 0, dy > 0 / dy < 0
 *
 * The two axis tests cannot both hold unless ax = ay = 0.  A tie on a boundary belongs to the axis sector.  The slope
 * 5/12 comes from the 5-12-13 triangle: it gives the axis sectors a half-width of atan(5/12) = 22.62 degrees, where
 * eight equal sectors would have 22.5; the diagonal sectors are 44.76 degrees wide.  All products fit in 32 bits
 * (12 * 65535 < 2^20).  Symmetries: (dx, dy) -> (-dy, dx) turns k into (k + 2) & 7; dx -> -dx into (4 - k) & 7;
 * dy -> -dy into (8 - k) & 7; the transpose into (2 - k) & 7.  On the boundaries: (12, 5) -> 0, (12, 6) -> 1,
 * (5, 12) -> 2, (3, 1) -> 0, (2, 1) -> 1, (65535, 27306) -> 0, (65535, 27307) -> 1.
 *
 * Direction test.  `allow` is a byte; bit k says that records of sector k may vote.  A record without a sector (zero
 * displacement) always passes: it has no direction to object to.  (It reaches the vote only where thr <= 0.)
 *
 * Per frame with side data:
 *   1. A record COUNTS iff it passes the bounds test of :262 — 0 <= dst_x >> shift < gw and m <= dst_y >> shift < gh - m
 *      — and the threshold of :251.
 *   2. rose[f].n[k] is the number of counting records of sector k, for every k, WHATEVER allow says.  Records without a
 *      sector are in no bin.
 *   3. A counting record votes for its destination cell iff it passes the direction test.
 *   4. From there on everything is :272-292 without the early return, exactly as mtgpu_scan_centres_device computes it
 *      — vn, vn == 0, the halo rows, out-of-grid neighbours — and gives centres[f] and
 *      flags[f] = centres[f] >= max(1, cn)  (:288).
 * A frame without side data (the scan's rule, :219-221; has_sd == NULL: the frame owns no record) reads 0 in every
 * output, rose included.
 *
 * Streams.  d_allow is n_streams bytes, one per stream; stream s owns frames [stream_off[s], stream_off[s + 1]), as in
 * mtgpu_zones.h.  A frame at or past stream_off[n_streams], or in front of stream_off[0], belongs to no stream and
 * reads 0 in every output.  Alternatively d_allow == NULL, d_stream_off == NULL and n_streams == 0: then the scalar
 * argument `allow`, in 0 .. 255, serves every frame.  With d_allow given, the scalar must still be in range and is not
 * used.
 *
 * Consequences (what the tests hold).
 *  A. allow == 0xFF gives the flags and centres of mtgpu_scan_centres_device bit for bit, for every vn and thr.
 *  B. rose does not depend on allow.  The sum of rose[f].n[k] over k is the number of counting records with non-zero
 *     displacement.
 *  C. Removal: take the same frame with every record whose sector is not allowed removed from the list, has_sd passed
 *     explicitly and unchanged; centres[f] equals the plain centre count of that frame.
 *  D. Rotation: replace every src by dst - (-dy, dx), where that stays inside int16.  Then rose'[(k + 2) & 7] = rose[k],
 *     and under allow' = rotl8(allow, 2) the centres do not change.  The mirror dx -> -dx does the same with the
 *     permutation (4 - k) & 7.
 *  E. Monotone: allow a subset of allow' implies centres(allow) <= centres(allow'), frame by frame.
 *  F. vn == 0 gives the plain centre scan, whatever allow is: no cell needs a vote.
 *
 * Out of scope: keep masks, blobs and compensation next to the direction test; the pipe, the C++ host layer and
 * mtgpu_scan_file (these, with the pipe's keep mask, are in mtgpu_pipe_dir.h); a per-cell allow plane; the sign of mt_mv.source — a compact record does not carry it, and the test
 * reads dst - src as the vote does; the row-banded grids (960x540 cells, 32767-wide grids: the class every sibling
 * rejects), which are MT_ERR_UNSUPPORTED with the grid named.
 *
 * Kernel (csrc/dir_kernels.hip): one workgroup per frame with side data; one tile of 32-bit vote counters in LDS; the
 * direction test is a handful of integer instructions per counting record, behind the branch the vote needs anyway; the
 * rose is counted per lane in registers and summed across each wave once per 131 072 records of a frame — no atomic per
 * record, no global atomics.  A bin is exact below 2^32 records.
 */
#ifndef MTGPU_DIR_H
#define MTGPU_DIR_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A frame's motion rose: the counting records per sector, 0 = E, clockwise on the screen (1 = SE, 2 = S, ... 7 = NE). */
typedef struct mt_dir_rose {
  uint32_t n[8];
} mt_dir_rose;                    /* 32 bytes, 4-byte aligned */

/* How the direction scan runs on a grid (src/motion_scanner.cpp:237-238: the analysed rows size the tile). */
typedef struct mtgpu_dir_plan {
  int32_t lds_bytes;              /* dynamic LDS per workgroup      */
  int32_t workgroup;              /* lanes                          */
  int32_t sectors;                /* 8                              */
  int32_t rose_bytes;             /* sizeof(mt_dir_rose) = 32       */
} mtgpu_dir_plan;

#define MTGPU_DIR_ALL 0xFF        /* every sector may vote: the plain centre scan */

/*
 * The plan mtgpu_scan_dir_device would pick for these parameters (the grid and the vertical margin of
 * src/motion_scanner.cpp:237-238 are all that matter) on a device with `lds_bytes_per_workgroup` of LDS per workgroup
 * (MI355X: 163840).  Pure host arithmetic: no HIP call, works without a device.  MT_ERR_INVALID: NULL / invalid
 * parameters, LDS size below 1024; MT_ERR_UNSUPPORTED (the grid is named): the tile and the mask plane do not fit.
 * out->lds_bytes <= lds_bytes_per_workgroup.
 */
int mtgpu_dir_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, mtgpu_dir_plan *out);

/*
 * The direction-filtered centre scan (src/motion_scanner.cpp:242-292 per frame, the vote of :262-268 only for records
 * of an allowed sector) and the roses of a device-resident batch; asynchronous on `stream`.  d_rec / rec_bytes /
 * n_records / d_frame_off / d_has_sd / n_frames as for mtgpu_scan_centres_device (rec_bytes 40 = mt_mv, 8 =
 * mt_mv_compact, 8-byte aligned).
 *   d_stream_off  n_streams + 1 uint64 frame offsets (device), non-decreasing, with d_allow; else NULL
 *   d_allow       n_streams bytes (device), or NULL with d_stream_off == NULL and n_streams == 0
 *   allow         0 .. 255; serves every frame when d_allow is NULL
 *   d_flags       n_frames uint8, or NULL;   d_centres   n_frames uint32, or NULL;   d_rose   n_frames mt_dir_rose, or NULL
 * Any one or two of the three outputs may be NULL (never touched then); all three NULL is MT_ERR_INVALID.  Every
 * element of every non-NULL output is written, and exactly n_frames of them.  n_frames == 0: MT_OK, nothing is
 * written.  MT_ERR_INVALID (the argument is named in mtgpu_last_error) for allow outside 0 .. 255, rec_bytes outside
 * {8, 40}, a misaligned pointer, NULL d_frame_off, d_allow given without d_stream_off / n_streams or the other way
 * round, and an output that is not memory of the context's device.  MT_ERR_UNSUPPORTED (the grid is named) as above.
 * Nothing is launched and no output byte is touched when the call fails this way.  Launch scratch (32 bytes per frame)
 * comes from the context's ring; with mtgpu_profile_enable on, the call records the same event triple as a scan launch.
 */
int mtgpu_scan_dir_device(mtgpu_ctx *ctx, const void *d_rec, int rec_bytes, uint64_t n_records,
                          const uint64_t *d_frame_off, const uint8_t *d_has_sd /* may be NULL */, uint32_t n_frames,
                          const uint64_t *d_stream_off, uint32_t n_streams, const uint8_t *d_allow, int32_t allow,
                          uint8_t *d_flags, uint32_t *d_centres, mt_dir_rose *d_rose, void *stream);

/*
 * The same for a batch in HOST memory (src/motion_scanner.cpp:217-295 for every frame, with the direction test ahead of
 * the vote): copies the records the offsets span, the offsets, has_sd, stream_off and the allow bytes to the device,
 * runs the call above, copies the outputs back; synchronous.  mv / frame_off / has_sd / n_frames as for
 * mtgpu_scan_frames_centres; stream_off: n_streams + 1 entries with allows: n_streams bytes, or both NULL and n_streams
 * 0; flags: n_frames uint8 or NULL; centres: n_frames uint32 or NULL; rose: n_frames mt_dir_rose or NULL.
 * MT_ERR_INVALID also for decreasing frame_off or stream_off and for stream_off[n_streams] != n_frames.
 */
int mtgpu_scan_frames_dir(mtgpu_ctx *ctx, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd,
                          uint32_t n_frames, const uint64_t *stream_off, uint32_t n_streams, const uint8_t *allows,
                          int32_t allow, uint8_t *flags, uint32_t *centres, mt_dir_rose *rose);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_DIR_H */
