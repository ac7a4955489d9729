/*
 * mtgpu_objects.h — object lists: the K largest blobs of every frame, ranked and boxed, and the number of blobs of a
 * minimum size.  Part of the C ABI of mtgpu.h, which includes this header (include either one).  Same conventions:
 * MT_* status codes, arguments validated before anything is launched, the `*_device` entry point takes device pointers
 * and is asynchronous on `stream`, the other takes host pointers and is synchronous; NO CPU fallback; no environment
 * variables.
 *
 * The blob scan (mtgpu_blobs.h) labels all blobs of a frame and reports one of them: the largest.  A second person
 * entering the picture is invisible while a larger object stands in it, and nothing counts the blobs that pass a
 * minimum size.  An object scan reports, per frame, a list — a size and a box for each of the k largest blobs, in a
 * defined order — and the rule "at least N things of at least M cells".
 *
 * Semantics.  The active plane, the centre cells C(f) (src/motion_scanner.cpp:272-294) and the blobs are exactly those
 * of mtgpu_blobs.h, without a keep mask (d_keep == NULL) and with one.  Beside the blob scan's arguments:
 *   k               1 .. MT_OBJECTS_MAX: the number of list entries per frame
 *   min_blob_cells  the least cell count of a blob that `objects` counts; values below 1 count as 1
 *   min_objects     the least `objects` for flags[f] = 1; values below 1 count as 1
 * Outputs, per frame f (each may be NULL, at least one must not be):
 *   list[f*k + j]   mt_object, j < k: the blob of rank j.  The order is `cells` descending, then `first` ascending;
 *                   every blob has a distinct `first`, so the order is total.  Ranks at or beyond blobs[f] read
 *                   {0, 0xFFFFFFFF, 0xFFFF x 4}
 *   objects[f]      uint32  the number of blobs with cells >= max(1, min_blob_cells), counted over ALL blobs of the
 *                   frame, not only the k listed ones
 *   centres[f], blobs[f]  uint32  as in the blob scan
 *   flags[f]        uint8   centres[f] >= max(1, clusters_needed) AND objects[f] >= max(1, min_objects)  (:288 with one
 *                   more term)
 * A frame without side data (the scan's rule, :219-221; has_sd == NULL: the frame owns no record) reads zeros and an
 * empty list; so does, under a mask, a frame at or behind stream_off[n_streams].  Every element of every non-NULL
 * output is written.
 *
 * Consequences.
 *  A. list[f*k + 0] is the blob scan's largest[f] and box[f], bit for bit, same tie rule (the blob that contains the
 *     smallest y * gw + x); centres and blobs are the blob scan's, without and with a mask.
 *  B. With min_objects <= 1, flags equals the blob scan's flags at the same min_blob_cells, bit for bit (one blob of
 *     min_blob_cells cells exists iff the largest has that many).
 *  C. The list for k is the first k entries of the list for MT_OBJECTS_MAX.
 *  D. The cells sum over all entries is at most centres; it equals centres when blobs <= k.  objects <= blobs.  objects
 *     equals the number of entries with cells >= min_blob_cells whenever that number is below k.
 *  E. For L >= 1 and clusters_needed <= 1: `objects`, handed to the unchanged mtgpu_sweep_streams_device as its
 *     d_centres with level L, gives the segments of mtgpu_merge_streams_device on `flags` at min_objects = L (objects
 *     >= 1 implies centres >= 1).  One scan answers every MIN_OBJECTS.
 *  F. Raising min_blob_cells raises no objects[f].  The list does not depend on min_blob_cells or min_objects.
 *
 * Kernel (csrc/objects_kernels.hip): one workgroup per frame with side data; up to the labels it is the blob scan's,
 * then a count over the roots, min(k, blobs) rounds of a 64-bit LDS maximum, one pass for all boxes and one 16-byte
 * store per entry.  LDS: the blob scan's layout plus MT_OBJECT_TABLE_BYTES per entry.  A grid for which that does not
 * fit — the grids mtgpu_blobs_preview refuses and, for large k, a few grids at its limit — is MT_ERR_UNSUPPORTED.
 *
 * Out of scope: there is no pipe form (mtgpu_pipe_*), no C++ host layer method, no mtgpu_scan_file option and no
 * compensated form (mtgpu_gmc_blobs.h) for object lists; no tracks across frames — the list of frame f says nothing
 * about which entry of frame f + 1 is the same object — and no per-object direction.  An object scan is a call on a
 * batch.
 */
#ifndef MTGPU_OBJECTS_H
#define MTGPU_OBJECTS_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MT_OBJECTS_MAX 16
/* LDS the ranking takes per list entry, behind the blob scan's layout: a 64-bit key and four 32-bit bounds */
#define MT_OBJECT_TABLE_BYTES 24

/* One blob of a frame's list. */
typedef struct mt_object {      /* 16 bytes, 16-byte aligned in the list */
  uint32_t cells;               /* cell count of the blob; 0: no such blob            */
  uint32_t first;               /* smallest y * grid_w + x of its cells (y: grid row) */
  uint16_t x0, y0, x1, y1;      /* inclusive cell bounds, as mt_blob_box              */
} mt_object;

/* How the object scan runs on a grid (src/motion_scanner.cpp:237-238: the analysed rows size the tile). */
typedef struct mtgpu_objects_plan {
  int32_t lds_bytes;              /* dynamic LDS per workgroup: mtgpu_blobs_preview's + k * MT_OBJECT_TABLE_BYTES */
  int32_t workgroup;              /* lanes                                             */
  int32_t keep_words_per_row;     /* W = (grid_w + 63) / 64                            */
  int32_t keep_words_per_stream;  /* grid_h * W: uint64 words of one stream's keep plane */
} mtgpu_objects_plan;

/*
 * The plan mtgpu_scan_objects_device would pick for these parameters (the grid and the vertical margin of
 * src/motion_scanner.cpp:237-238 are all that matter) and `k` list entries on a device with `lds_bytes_per_workgroup`
 * of LDS per workgroup (MI355X: 163840), and the sizes of a keep mask.  Pure host arithmetic: no HIP call, works
 * without a device.  MT_ERR_INVALID: k outside 1 .. MT_OBJECTS_MAX, NULL / invalid parameters, LDS size below 1024;
 * MT_ERR_UNSUPPORTED (the grid is named): the layout does not fit.  out->lds_bytes <= lds_bytes_per_workgroup.
 */
int mtgpu_objects_preview(const mt_scan_params *p, int k, int lds_bytes_per_workgroup, mtgpu_objects_plan *out);

/*
 * The object scan (src/motion_scanner.cpp:272-294 per frame — :282 ANDed with the stream's keep bit where a mask is
 * given — then the components of the centres, ranked) of a device-resident batch; asynchronous on `stream`.  d_rec /
 * rec_bytes / n_records / d_frame_off / d_has_sd / n_frames / d_stream_off / n_streams / d_keep as for
 * mtgpu_scan_blobs_device.
 *   d_flags n_frames uint8; d_centres, d_blobs, d_objects n_frames uint32 each; d_list n_frames * k mt_object, 16-byte
 *   aligned; each or NULL
 * All five outputs NULL is MT_ERR_INVALID; a NULL output is never touched.  n_frames == 0: MT_OK, nothing is written.
 * MT_ERR_INVALID (the argument is named in mtgpu_last_error) for k outside 1 .. MT_OBJECTS_MAX, rec_bytes outside
 * {8, 40}, a misaligned pointer, NULL d_frame_off, d_keep given with d_stream_off == NULL or n_streams == 0, d_keep ==
 * NULL with d_stream_off given or n_streams != 0, and an output or d_keep that is not memory of the context's device.
 * MT_ERR_UNSUPPORTED (the grid is named) as above.  Nothing is launched and no output byte is touched when the call
 * fails this way.  Launch scratch (32 bytes per frame) comes from the context's ring; with mtgpu_profile_enable on, the
 * call records the same event triple as a scan launch.
 */
int mtgpu_scan_objects_device(mtgpu_ctx *ctx, const void *d_rec, int rec_bytes, uint64_t n_records,
                              const uint64_t *d_frame_off, const uint8_t *d_has_sd /* may be NULL */, uint32_t n_frames,
                              const uint64_t *d_stream_off /* NULL iff d_keep is NULL */, uint32_t n_streams,
                              const uint64_t *d_keep /* NULL: no mask */, int32_t k, int32_t min_blob_cells,
                              int32_t min_objects, uint8_t *d_flags, uint32_t *d_centres, uint32_t *d_blobs,
                              uint32_t *d_objects, mt_object *d_list, void *stream);

/*
 * The same for a batch in HOST memory (src/motion_scanner.cpp:217-295 for every frame, then the components of the
 * centres, ranked): copies the records the offsets span, the offsets, has_sd, stream_off and keep to the device, runs
 * the call above, copies the outputs back; synchronous.  mv / frame_off / has_sd / n_frames / stream_off / n_streams /
 * keep as for mtgpu_scan_frames_blobs; `list` needs no alignment here.  MT_ERR_INVALID also for decreasing frame_off or
 * stream_off and for stream_off[n_streams] != n_frames.
 */
int mtgpu_scan_frames_objects(mtgpu_ctx *ctx, const mt_mv *mv, const uint64_t *frame_off, const uint8_t *has_sd,
                              uint32_t n_frames, const uint64_t *stream_off, uint32_t n_streams, const uint64_t *keep,
                              int32_t k, int32_t min_blob_cells, int32_t min_objects, uint8_t *flags, uint32_t *centres,
                              uint32_t *blobs, uint32_t *objects, mt_object *list);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_OBJECTS_H */
