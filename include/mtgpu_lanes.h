/*
 * mtgpu_lanes.h — direction planes: the direction scan of mtgpu_dir.h with one allow byte per grid cell, and the flow map
 * such a plane is learned from.  Part of the C ABI of mtgpu.h, which includes this header (include either one).  Same
 * conventions: MT_* status codes, arguments validated before anything is launched, the `*_device` entry points take
 * device pointers and are asynchronous on `stream`, the others take host pointers and are synchronous; NO CPU fallback;
 * no environment variables.
 *
 * The direction filter has one answer to "which way may things move" for the whole picture.  That covers a one-way
 * street.  A two-way road wants E in the near lane and W in the far one, and the event is a car going E in the far
 * lane; a gate beside a pavement wants arrivals at the gate and everything on the pavement; a conveyor across a hall
 * makes W ordinary on the belt and an event anywhere else.  A zone (mtgpu_zones.h) blinds cells; one allow byte cannot
 * say "W here, E there".  The decision is per record, ahead of the vote, and the vote's tile lives only in a kernel's
 * LDS: no chain of the existing calls gives it.
 *
 * Semantics.  Everything is integer and exact.  Everything not restated here is mtgpu_dir.h's, word for word: the
 * COUNTING record (bounds test and threshold), the sector rule 12 ay <= 5 ax with ties going to the axis sector, the
 * record without a sector, frames without side data, stream ownership by stream_off, and frames in front of the first
 * stream or behind the last one, which read 0 everywhere.
 *
 * Plane scan.  A plane is gh x gw bytes, row-major: plane[y * gw + x] is the allow byte of cell (x, y).
 *   1. A counting record with sector k and destination cell (gx, gy) = (dst_x >> shift, dst_y >> shift) votes iff bit k
 *      of plane[gy * gw + gx] is set.  A counting record without a sector always votes.
 *   2. rose[f] is the direction scan's: every counting record per sector, whatever the plane says.
 *   3. From the votes on everything is the centre scan: centres[f], flags[f] = centres[f] >= max(1, cn).
 *   4. Bytes of cells outside the analysed rows are never read.
 * Planes come in one of two forms.  d_planes is n_streams x gh x gw bytes and stream s uses plane s: this form comes
 * with d_stream_off and n_streams > 0.  Or d_planes is ONE plane serving every frame: this form comes with
 * d_stream_off == NULL and n_streams == 0.  d_planes == NULL is MT_ERR_INVALID.  A plane has no alignment: plane s
 * begins s * gh * gw bytes behind plane 0, wherever that falls.
 *
 * Flow map.  d_flow[((s * 8 + k) * gh + y) * gw + x] (uint32) is the number of counting records of sector k with
 * destination cell (x, y), over the frames of stream s that have side data.  Rows outside the analysed range read 0.
 * The call clears, then counts.  A frame outside every stream counts nowhere.  The maps are integers and add across
 * batches.
 *
 * Consequences (what the tests hold).
 *  A. A plane filled with one byte b gives the flags, centres and rose of mtgpu_scan_dir_device(allow = b) bit for bit;
 *     per-stream uniform planes give those of its per-stream bytes.
 *  B. A plane of 0xFF is mtgpu_scan_centres_device.
 *  C. Removal: delete every record whose sector its destination cell forbids; the plain centre count of what is left
 *     equals centres[f].
 *  D. Monotone: plane a subset of plane' bitwise in every cell implies centres <= centres', frame by frame.
 *  E. Zones tie: with vn >= 1, thr >= 1 and every byte in {0x00, 0xFF}, centres equal the masked count of
 *     mtgpu_scan_zones_device under keep = (byte == 0xFF).
 *  F. vn == 0 gives the plain centre scan, whatever the plane holds: no cell needs a vote.
 *  G. For every stream and every k, the sum of flow[s][k] over its cells equals the sum of rose[f].n[k] over its frames.
 *     The flow map depends on neither the launch grid nor the order in which workgroups arrive.
 *
 * Out of scope: the pipe, the C++ host layer and mtgpu_scan_file (these, with the pipe's keep mask, are in
 * mtgpu_pipe_lanes.h); planes next to keep masks on a resident batch, blobs or compensation; a
 * min_centres filter on the flow map; the row-banded grids (960x540 cells, 32767-wide grids: the class every sibling
 * rejects), which are MT_ERR_UNSUPPORTED with the grid named.
 *
 * Kernels (csrc/lanes_kernels.hip).  The plane scan is the direction scan's kernel with the byte looked up per counting
 * record, behind the branch on bounds and threshold that the vote needs anyway: a record that does not count costs what
 * it costs there.  STAGED form: the workgroup first copies the analysed rows of its stream's plane into LDS behind the
 * direction scan's areas, and the per-record read is one LDS byte.  Unstaged form, where those bytes do not fit next to
 * the tile: the byte is a plain cached global load.  Sizes, MI355X (163 840 bytes of LDS per workgroup):
 *
 *     grid                                   direction scan   plane rows          total
 *     1080p defaults (120 x 68, margin 3)            31 792   62 x 120 =  7 440    39 232   staged, still two workgroups per CU
 *     4K, margin 6 (240 x 135)                      124 048   123 x 240 = 29 520  153 568   staged
 *     4K, margin 0                                  135 952   135 x 240 = 32 400  168 352 > 163 840: unstaged, at 135 952
 *
 * The flow map has no tile: one no-return global atomic add per counting record with a sector, as the activity map's
 * flush uses them; integer adds commute, which is consequence G's second sentence.
 */
#ifndef MTGPU_LANES_H
#define MTGPU_LANES_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mt_dir_rose (mtgpu_dir.h), by its struct tag: whichever of the two headers is read first, the prototypes below
 * compile; its definition is in scope for every includer of either. */
struct mt_dir_rose;

/* How the plane scan runs on a grid (src/motion_scanner.cpp:237-238: the analysed rows size the tile and the staged rows). */
typedef struct mtgpu_lanes_plan {
  int32_t lds_bytes;              /* dynamic LDS per workgroup                                          */
  int32_t workgroup;              /* lanes                                                              */
  int32_t staged;                 /* 1: the plane's analysed rows are held in LDS; 0: read from memory  */
  int32_t plane_bytes;            /* gw * gh: one plane                                                 */
} mtgpu_lanes_plan;

/*
 * The plan mtgpu_scan_lanes_device would pick for these parameters (the grid and the vertical margin of
 * src/motion_scanner.cpp:237-238 are all that matter) on a device with `lds_bytes_per_workgroup` of LDS per workgroup
 * (MI355X: 163840).  Pure host arithmetic: no HIP call, works without a device.  MT_ERR_INVALID: NULL / invalid
 * parameters, LDS size below 1024; MT_ERR_UNSUPPORTED (the grid is named): the direction scan's tile and mask plane do
 * not fit.  out->lds_bytes <= lds_bytes_per_workgroup.
 */
int mtgpu_lanes_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, mtgpu_lanes_plan *out);

/*
 * The plane-filtered centre scan (src/motion_scanner.cpp:242-292 per frame, the vote of :262-268 only for records whose
 * sector the destination cell's byte allows) and the roses of a device-resident batch; asynchronous on `stream`.
 * d_rec / rec_bytes / n_records / d_frame_off / d_has_sd / n_frames as for mtgpu_scan_dir_device.
 *   d_stream_off  n_streams + 1 uint64 frame offsets (device), non-decreasing, with per-stream planes; else NULL
 *   n_streams     > 0 with d_stream_off; 0 without
 *   d_planes      n_streams x gh x gw bytes (device), or gh x gw bytes with d_stream_off == NULL; never NULL
 *   d_flags       n_frames uint8, or NULL;   d_centres   n_frames uint32, or NULL;   d_rose   n_frames mt_dir_rose, or NULL
 * Any one or two of the three outputs may be NULL (never touched then); all three NULL is MT_ERR_INVALID.  Every
 * element of every non-NULL output is written, and exactly n_frames of them.  n_frames == 0: MT_OK, nothing is
 * written.  MT_ERR_INVALID (the argument is named in mtgpu_last_error) for NULL d_planes, rec_bytes outside {8, 40}, a
 * misaligned pointer, NULL d_frame_off, d_stream_off given with n_streams 0 or the other way round, and an output that
 * is not memory of the context's device.  MT_ERR_UNSUPPORTED (the grid is named) as above.  Nothing is launched and no
 * output byte is touched when the call fails this way.  Launch scratch (32 bytes per frame) comes from the context's
 * ring; with mtgpu_profile_enable on, the call records the same event triple as a scan launch.
 */
int mtgpu_scan_lanes_device(mtgpu_ctx *ctx, const void *d_rec, int rec_bytes, uint64_t n_records,
                            const uint64_t *d_frame_off, const uint8_t *d_has_sd /* may be NULL */, uint32_t n_frames,
                            const uint64_t *d_stream_off, uint32_t n_streams, const uint8_t *d_planes, uint8_t *d_flags,
                            uint32_t *d_centres, struct mt_dir_rose *d_rose, void *stream);

/*
 * The same for a batch in HOST memory (src/motion_scanner.cpp:217-295 for every frame, with the plane's test ahead of
 * the vote): copies the records the offsets span, the offsets, has_sd, stream_off and the planes to the device, runs
 * the call above, copies the outputs back; synchronous.  mv / frame_off / has_sd / n_frames as for
 * mtgpu_scan_frames_dir; stream_off: n_streams + 1 entries with planes: n_streams x gh x gw bytes, or stream_off NULL,
 * n_streams 0 and planes: gh x gw bytes.  MT_ERR_INVALID also for decreasing frame_off or stream_off and for
 * stream_off[n_streams] != n_frames.
 */
int mtgpu_scan_frames_lanes(mtgpu_ctx *ctx, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd,
                            uint32_t n_frames, const uint64_t *stream_off, uint32_t n_streams, const uint8_t *planes,
                            uint8_t *flags, uint32_t *centres, struct mt_dir_rose *rose);

/*
 * The flow map of a device-resident batch (the counting records of src/motion_scanner.cpp:246-262, per stream, sector
 * and destination cell); asynchronous on `stream`.  d_rec / rec_bytes / n_records / d_frame_off / d_has_sd / n_frames as
 * above.
 *   d_stream_off  n_streams + 1 uint64 frame offsets (device), non-decreasing; required
 *   d_flow        n_streams x 8 x gh x gw uint32; memory of the context's device (global atomics)
 * Every element of d_flow is written: the call clears, then counts.  n_streams == 0: MT_OK, nothing is written.
 * MT_ERR_INVALID (the argument is named) for NULL d_flow, NULL d_stream_off, rec_bytes outside {8, 40}, a misaligned
 * pointer, NULL d_frame_off with frames, and a d_flow that is not memory of the context's device.  MT_ERR_UNSUPPORTED
 * (the grid is named) for the grids the plane scan rejects.  Nothing is launched and no output byte is touched when the
 * call fails this way.
 */
int mtgpu_flow_map_device(mtgpu_ctx *ctx, const void *d_rec, int rec_bytes, uint64_t n_records, const uint64_t *d_frame_off,
                          const uint8_t *d_has_sd /* may be NULL */, uint32_t n_frames, const uint64_t *d_stream_off,
                          uint32_t n_streams, uint32_t *d_flow, void *stream);

/*
 * The same for a batch in HOST memory (src/motion_scanner.cpp:246-262 for every record of every frame with side data):
 * copies the batch to the device, runs the call above, copies the map back; synchronous.  stream_off: n_streams + 1
 * entries, required; flow: n_streams x 8 x gh x gw uint32.  MT_ERR_INVALID also for decreasing frame_off or stream_off
 * and for stream_off[n_streams] != n_frames.
 */
int mtgpu_flow_map(mtgpu_ctx *ctx, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd, uint32_t n_frames,
                   const uint64_t *stream_off, uint32_t n_streams, uint32_t *flow);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_LANES_H */
