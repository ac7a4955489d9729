/*
 * mtgpu_headings.h — object headings: the rose and the summed displacement of every listed object.  Part of the C ABI of
 * mtgpu.h, which includes this header (include either one).  Same conventions: MT_* status codes, arguments validated
 * before anything is launched, the `*_device` entry point takes device pointers and is asynchronous on `stream`, the
 * other takes host pointers and is synchronous; NO CPU fallback; no environment variables.
 *
 * The object scan (mtgpu_objects.h) says how many objects a frame holds, the tracks pass (mtgpu_tracks.h) how long each
 * has existed, the direction scan (mtgpu_dir.h) which way a frame's records move.  None says which way an OBJECT moves:
 * the direction scan's rose is one histogram per frame — a car going E and a walker going W give one rose with two
 * lobes, and nothing assigns a lobe to a box — and the direction filter judges single records, so a blob of 30 cells
 * whose records point E, with three noisy records pointing W, cannot be judged as a whole.  The heading scan is the
 * object scan plus, for each of the k listed blobs, the motion of the records that land in it.
 *
 * Semantics.  Everything is integer and exact.  The grid, the active plane, the centre cells (src/motion_scanner.cpp:
 * 272-294), the blobs, their order and the keep mask are those of mtgpu_objects.h.  "Counting record" (the bounds test
 * of :262 and the threshold of :251), dx = dst_x - src_x, dy = dst_y - src_y and "sector" (the 5-12-13 rule; a zero
 * displacement has no sector) are those of mtgpu_dir.h.
 *
 * A record BELONGS TO entry j of frame f iff it is a counting record of f and its destination cell
 * (dst_x >> shift, dst_y >> shift) is a cell of the blob of rank j.  Cells of blobs are centre cells, hence active and,
 * under a mask, kept; no further mask term is needed.  These records belong to no entry: records in active cells that
 * are no centre (column 0 and gw - 1, isolated cells), records in blobs of rank k or beyond, records that do not count.
 *
 * Arguments beside the object scan's:
 *   allow           0 .. 255, one byte for the call: bit s admits an object of heading s
 *   min_objects     at most k (MT_ERR_INVALID otherwise); values below 1 count as 1
 * Outputs, per frame f (each may be NULL, at least one must not be; a NULL output is never touched; every element of a
 * non-NULL output is written):
 *   flags, centres, blobs, objects, list   as in the object scan, except that flags uses the rule below
 *   motion[f*k + j]  mt_heading, j < k: the motion of entry j.  An entry with no blob — at or beyond blobs[f], a frame
 *                   without side data, a frame behind the last stream — reads all zeros with heading = MT_HEADING_NONE
 *   allowed[f]      uint32  the number of listed entries with cells >= max(1, min_blob_cells) whose heading is
 *                   MT_HEADING_NONE or has its bit set in `allow`.  A still object has no direction to object to, as in
 *                   mtgpu_dir.h
 *   flags[f]        uint8   centres[f] >= max(1, clusters_needed) AND allowed[f] >= max(1, min_objects)
 *
 * Consequences (what the tests hold).
 *  A. centres, blobs, objects and list are mtgpu_scan_objects_device's, bit for bit, with and without a mask, for both
 *     record sizes.
 *  B. With allow == 0xFF, allowed[f] == min(objects[f], k): the list is sorted by cells, so the entries counted are a
 *     prefix.  With min_objects <= k, which the call enforces, flags are the object scan's flags bit for bit.
 *  C. motion does not depend on allow, min_blob_cells or min_objects.  motion for k is the first k entries per frame of
 *     motion for MT_OBJECTS_MAX.
 *  D. sum(n) <= records.  With 1 <= vectors_needed <= 255, records >= cells * vectors_needed: every centre cell is
 *     active.  Without a mask, the sum over a frame's entries of n[s] is at most rose[f].n[s] of mtgpu_scan_dir_device;
 *     it is equal when every counting record of the frame lands in a listed blob.
 *  E. Quarter turn: replace every src by dst - (-dy, dx), where that stays inside int16.  Then list is unchanged,
 *     n'[(s + 2) & 7] = n[s], sum_dx' = -sum_dy, sum_dy' = sum_dx and, where the maximum of n is unique,
 *     heading' = (heading + 2) & 7.
 *  F. allow a subset of allow' implies allowed <= allowed', frame by frame.  For clusters_needed <= 1, `allowed` handed
 *     to the unchanged mtgpu_sweep_streams_device as its d_centres with level L gives the segments of
 *     mtgpu_merge_streams_device on `flags` at min_objects = L.
 *
 * Kernel (csrc/headings_kernels.hip): one workgroup per frame with side data; up to the boxes it is the object scan's.
 * Then the labels of the listed blobs' cells become ranks, the frame's records stream a second time — a record that
 * belongs adds to its entry's bin, count and two 64-bit sums in LDS — and lane j stores entry j with four 16-byte
 * stores.  A frame without a centre leaves before the second pass: quiet frames read their records once.  LDS: the
 * object scan's layout plus MT_HEADING_TABLE_BYTES per entry.  A grid for which that does not fit — the grids
 * mtgpu_objects_preview refuses and, for large k, a few grids at its limit — is MT_ERR_UNSUPPORTED.
 *
 * Out of scope: per-stream allow bytes; a compensated form (mtgpu_gmc_blobs.h); the pipe (mtgpu_pipe_*), the C++ host
 * layer and mtgpu_scan_file; velocity prediction in the tracks pass — sum_dx / records is what it would read; the
 * row-banded grids, which are MT_ERR_UNSUPPORTED as in every sibling.  A heading scan is a call on a batch.  (This
 * header is the per-object direction that mtgpu_objects.h names as out of its scope.)
 */
#ifndef MTGPU_HEADINGS_H
#define MTGPU_HEADINGS_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mt_object of mtgpu_objects.h: named as a struct here, so that either header may be the first one included */
struct mt_object;

#define MT_HEADING_NONE 0xFFFFFFFFu
/* LDS the motion table takes per list entry, behind the object scan's layout: eight 32-bit bins, a 32-bit record
 * count, a pad word and two 64-bit sums */
#define MT_HEADING_TABLE_BYTES 56

/* The motion of one entry of a frame's list. */
typedef struct mt_heading {     /* 64 bytes, 16-byte aligned in the array */
  uint32_t n[8];                /* belonging records per sector, 0 = E, clockwise; records without a sector are in no bin */
  uint32_t records;             /* all belonging records, the still ones included */
  uint32_t heading;             /* the sector with the largest n[], the LOWEST such sector on a tie; MT_HEADING_NONE iff every n[] is 0 */
  int64_t sum_dx;               /* sum of dx over the belonging records */
  int64_t sum_dy;               /* sum of dy over the belonging records */
  uint64_t reserved;            /* 0 */
} mt_heading;

/* How the heading scan runs on a grid (src/motion_scanner.cpp:237-238: the analysed rows size the tile). */
typedef struct mtgpu_headings_plan {
  int32_t lds_bytes;              /* dynamic LDS per workgroup: mtgpu_objects_preview's + k * MT_HEADING_TABLE_BYTES */
  int32_t workgroup;              /* lanes                                             */
  int32_t keep_words_per_row;     /* W = (grid_w + 63) / 64                            */
  int32_t keep_words_per_stream;  /* grid_h * W: uint64 words of one stream's keep plane */
} mtgpu_headings_plan;

/*
 * The plan mtgpu_scan_headings_device would pick for these parameters (the grid and the vertical margin of
 * src/motion_scanner.cpp:237-238 are all that matter) and `k` list entries on a device with `lds_bytes_per_workgroup`
 * of LDS per workgroup (MI355X: 163840), and the sizes of a keep mask.  Pure host arithmetic: no HIP call, works
 * without a device.  MT_ERR_INVALID: k outside 1 .. MT_OBJECTS_MAX, NULL / invalid parameters, LDS size below 1024;
 * MT_ERR_UNSUPPORTED (the grid is named): the layout does not fit.  out->lds_bytes <= lds_bytes_per_workgroup.
 */
int mtgpu_headings_preview(const mt_scan_params *p, int k, int lds_bytes_per_workgroup, mtgpu_headings_plan *out);

/*
 * The heading scan (src/motion_scanner.cpp:272-294 per frame — :282 ANDed with the stream's keep bit where a mask is
 * given — then the components of the centres, ranked, then the records of :246-268 once more, per listed blob) of a
 * device-resident batch; asynchronous on `stream`.  d_rec / rec_bytes / n_records / d_frame_off / d_has_sd / n_frames /
 * d_stream_off / n_streams / d_keep / k / min_blob_cells as for mtgpu_scan_objects_device.
 *   d_flags n_frames uint8; d_centres, d_blobs, d_objects, d_allowed n_frames uint32 each; d_list n_frames * k
 *   mt_object and d_motion n_frames * k mt_heading, 16-byte aligned; each or NULL
 * All seven outputs NULL is MT_ERR_INVALID; a NULL output is never touched.  n_frames == 0: MT_OK, nothing is written.
 * MT_ERR_INVALID (the argument is named in mtgpu_last_error) for k outside 1 .. MT_OBJECTS_MAX, min_objects above k,
 * allow outside 0 .. 255, rec_bytes outside {8, 40}, a misaligned pointer, NULL d_frame_off, d_keep given with
 * d_stream_off == NULL or n_streams == 0, d_keep == NULL with d_stream_off given or n_streams != 0, and an output or
 * d_keep that is not memory of the context's device.  MT_ERR_UNSUPPORTED (the grid is named) as above.  Nothing is
 * launched and no output byte is touched when the call fails this way.  Launch scratch (32 bytes per frame) comes from
 * the context's ring; with mtgpu_profile_enable on, the call records the same event triple as a scan launch.
 */
int mtgpu_scan_headings_device(mtgpu_ctx *ctx, const void *d_rec, int rec_bytes, uint64_t n_records,
                               const uint64_t *d_frame_off, const uint8_t *d_has_sd /* may be NULL */, uint32_t n_frames,
                               const uint64_t *d_stream_off /* NULL iff d_keep is NULL */, uint32_t n_streams,
                               const uint64_t *d_keep /* NULL: no mask */, int32_t k, int32_t min_blob_cells,
                               int32_t min_objects, int32_t allow, uint8_t *d_flags, uint32_t *d_centres,
                               uint32_t *d_blobs, uint32_t *d_objects, struct mt_object *d_list, mt_heading *d_motion,
                               uint32_t *d_allowed, void *stream);

/*
 * The same for a batch in HOST memory (src/motion_scanner.cpp:217-295 for every frame, then the components of the
 * centres, ranked, then the records once more): copies the records the offsets span, the offsets, has_sd, stream_off and
 * keep to the device, runs the call above, copies the outputs back; synchronous.  mv / frame_off / has_sd / n_frames /
 * stream_off / n_streams / keep as for mtgpu_scan_frames_objects; `list` and `motion` need no alignment here.
 * MT_ERR_INVALID also for decreasing frame_off or stream_off and for stream_off[n_streams] != n_frames.
 */
int mtgpu_scan_frames_headings(mtgpu_ctx *ctx, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd,
                               uint32_t n_frames, const uint64_t *stream_off, uint32_t n_streams, const uint64_t *keep,
                               int32_t k, int32_t min_blob_cells, int32_t min_objects, int32_t allow, uint8_t *flags,
                               uint32_t *centres, uint32_t *blobs, uint32_t *objects, struct mt_object *list,
                               mt_heading *motion, uint32_t *allowed);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_HEADINGS_H */
