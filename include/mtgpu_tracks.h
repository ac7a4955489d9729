/*
 * mtgpu_tracks.h — object tracks: which entry of the previous motion frame's object list each listed object continues,
 * how long it has existed, which track it belongs to and how long that track gets.  Part of the C ABI of mtgpu.h, which
 * includes this header (include either one).  Same conventions: MT_* status codes, arguments validated before anything
 * is launched, the `*_device` entry point takes device pointers and is asynchronous on `stream`, the other takes host
 * pointers and is synchronous; NO CPU fallback; no environment variables.
 *
 * An object scan (mtgpu_objects.h) gives every frame a ranked list of its k largest blobs; persistence
 * (mtgpu_persist.h) follows ONE box per frame, the largest blob.  A parked lorry that sways all day keeps every frame's
 * run alive, and nothing tells that the small object beside it has existed for two frames.  This call links the lists:
 * it adds the rule "keep a frame only if one of its objects belongs to a track of at least MIN_TRACK frames".
 *
 * Semantics (everything is integer and exact).  The input is a batch of n_frames frames in S = n_streams streams
 * (stream_off: S + 1 frame offsets, as in mtgpu_persist_flags_device).  Each frame has flags[f], optionally has_sd[f],
 * and list[f*k + j], an mt_object for j < k, k in 1 .. MT_OBJECTS_MAX, in the layout the object scan writes.
 *
 * Frame classes inside a stream:
 *   M   flags[f] != 0.
 *   T   (transparent) otherwise, has_sd != NULL && has_sd[f] == 0.  These are key frames: they were never analysed and
 *       must not break a run.  Without this rule every GOP ends every run.
 *   Q   otherwise: the frame was analysed and was quiet.
 * For an M frame f:
 *   p(f)    the previous M frame of the same stream, or none.
 *   q(f)    the number of Q frames strictly between p(f) and f.
 *
 * Present entries.  Entry (f, j) is PRESENT iff f is an M frame and list[f*k + j].cells >= max(1, min_cells).  The
 * object scan's order makes the present entries a prefix; the call does not rely on that: an unsorted list is legal
 * input and every rule below is per entry.
 *
 * Predecessor.  For a present entry (f, j), pred(f, j) is
 *   none                if p(f) is none or q(f) > max_dropout;
 *   otherwise           the smallest i for which (p(f), i) is present and linked(box(p(f), i), box(f, j)) holds;
 *   none                if no such i exists.
 * linked(A, B) is persistence's predicate on the four bounds: false if either box is all 0xFFFF, and otherwise true iff
 *   B.x0 <= A.x1 + reach,  A.x0 <= B.x1 + reach,  B.y0 <= A.y1 + reach,  A.y0 <= B.y1 + reach
 * in arithmetic of at least 32 bits; reach is in [0, 65535].
 * The predecessor depends on two lists and on nothing earlier.  It is not a matching: two entries may share a
 * predecessor (a split), and an entry linked to several picks the lowest rank (a merge follows the larger object).
 *
 * Derived quantities, for a present entry:
 *   age(f, j)   1 if pred is none, else age(p(f), pred) + 1.
 *   id(f, j)    f*k + j (f: the frame's index in the batch) if pred is none, else id(p(f), pred).
 *   A track is a root (a present entry without predecessor) and everything that descends from it.
 *   len(f, j)   the largest age over all entries with the same id: the depth of the track's tree.
 *
 * Outputs (each may be NULL, not all of them; every element of every non-NULL output is written):
 *   pred[f*k + j]   uint8    index of the predecessor, 0xFF (MT_TRACK_NO_PRED) for none
 *   age[f*k + j]    uint32   as above
 *   id[f*k + j]     uint32   as above
 *   len[f*k + j]    uint32   as above
 *   track[f]        uint32   the largest len over the frame's present entries, or 0
 *   flags_out[f]    uint8    flags[f] != 0 && track[f] >= max(1, min_track), written as 0 / 1
 * An entry that is not present reads pred = 0xFF, age = len = 0 and id = 0xFFFFFFFF (MT_TRACK_NO_ID).  Frames outside
 * [stream_off[0], stream_off[S]) read the same, and their track[f] and flags_out[f] read 0.
 *
 * Limit: n_frames * k must be below 0xFFFFFFFF, else MT_ERR_INVALID.
 *
 * Consequences.
 *  A. k = 1, min_cells <= 1, and every M frame has list[f].cells > 0: age[f] == pos[f], len[f] == track[f] == run[f],
 *     and flags_out equals that of mtgpu_persist_flags_device on the same flags and has_sd, with box[f] set to the
 *     entry's bounds and min_run = min_track — bit for bit.  Where an M frame's entry is absent the two differ:
 *     persistence counts a run of 1 for that frame, this call gives track = 0.
 *  B. For present entries: pred == 0xFF iff age == 1; len >= age; len is constant over a track; for each root,
 *     len[root] equals the largest age carrying its id.  The number of roots is the number of tracks.
 *  C. For a level L >= 1: `track`, handed to the unchanged mtgpu_sweep_streams_device as its d_centres with levels =
 *     {L, ...}, gives the segments of mtgpu_merge_streams_device on flags_out at min_track = L, bit for bit.  One pass
 *     answers every MIN_TRACK.
 *  D. A stream's outputs from a call on that stream alone, with the stream's first frame times k added to every id
 *     (other than MT_TRACK_NO_ID), equal that stream's outputs in the whole batch.
 *  E. pred depends on reach, max_dropout, min_cells and the two lists only.  Raising max_dropout turns no pred into
 *     none.  There is NO monotony in reach for age: a wider reach can swap a predecessor for a lower-ranked, younger
 *     one.
 *
 * Out of scope: exclusive (one-to-one) assignment; velocity prediction; per-object direction; the pipe, the C++ host
 * layer and mtgpu_scan_file (tracking takes pooled per-frame results, as persistence does: on the decode path it runs
 * once per recording); a compensated form.
 *
 * Kernels (csrc/tracks_kernels.hip): a clear kernel; then one workgroup per stream that walks the stream forwards in
 * tiles of frames_per_tile frames, sixteen lanes to a frame, one lane to a list entry — persistence's scan finds p(f)
 * and q(f), sixteen width-16 shuffles find the predecessor, a scan whose element is a map spread over sixteen lanes
 * gives ages and ids, and one atomic maximum per chain of a track records the depth by root; then a finish kernel,
 * parallel over the frames, reads the depth back.  A long stream is NOT split over several workgroups.
 */
#ifndef MTGPU_TRACKS_H
#define MTGPU_TRACKS_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MT_TRACK_NO_PRED 0xFFu
#define MT_TRACK_NO_ID 0xFFFFFFFFu

/* mt_object (mtgpu_objects.h), by its struct tag: whichever of the two headers is included first, mtgpu.h reaches this
 * one before or after that header's own body, so the prototypes below cannot rely on the typedef. */
struct mt_object;

/* How the tracks pass runs. */
typedef struct mtgpu_tracks_plan {
  int32_t workgroup;             /* lanes */
  int32_t frames_per_tile;       /* frames a workgroup takes per step */
  int32_t work_words_per_entry;  /* uint32 words of d_work per list entry: d_work holds this * n_frames * k words */
} mtgpu_tracks_plan;

/* The plan of mtgpu_track_objects_device for k entries per frame: workgroup is a multiple of 64, frames_per_tile *
 * MT_OBJECTS_MAX a multiple of workgroup.  Pure host, no device.  MT_ERR_INVALID: out is NULL, k outside
 * 1 .. MT_OBJECTS_MAX. */
int mtgpu_tracks_preview(int k, mtgpu_tracks_plan *out);

/*
 * The tracks of a device-resident batch; asynchronous on `stream`.
 *   d_flags       n_frames uint8                            d_has_sd   n_frames uint8 or NULL
 *   d_list        n_frames * k mt_object, 16-byte aligned   d_stream_off   n_streams + 1 uint64, non-decreasing; entries
 *                                                           above n_frames are read as n_frames
 *   d_work        work_words_per_entry * n_frames * k uint32: the caller's workspace, in the d_work idiom of
 *                 mtgpu_persist_flags_device (the depth table by root, and the ids when d_id is NULL).  Its contents
 *                 are unspecified afterwards.  The call allocates nothing and takes nothing from the context's scratch
 *                 ring.
 *   d_pred        n_frames * k uint8; d_age, d_id, d_len n_frames * k uint32 each; d_track n_frames uint32; d_flags_out
 *                 n_frames uint8; each or NULL
 * MT_ERR_INVALID (the argument is named in mtgpu_last_error) for: all six outputs NULL; k outside 1 .. MT_OBJECTS_MAX;
 * n_frames * k at or above 0xFFFFFFFF; reach > 65535; NULL d_flags, d_list, d_stream_off or d_work with n_frames > 0;
 * n_streams == 0 with n_frames > 0; a misaligned pointer; an output or d_work that is not memory of the context's
 * device; an output or d_work whose byte range overlaps an input's or another output's — there is NO in-place form.
 * n_frames == 0: MT_OK, and nothing is touched.  Nothing is launched and no byte is written when a call fails this way.
 */
int mtgpu_track_objects_device(mtgpu_ctx *ctx, const uint8_t *d_flags, const uint8_t *d_has_sd /* may be NULL */,
                               const struct mt_object *d_list, int32_t k, uint32_t n_frames, const uint64_t *d_stream_off,
                               uint32_t n_streams, uint32_t min_cells, uint32_t max_dropout, uint32_t reach,
                               uint32_t min_track, uint32_t *d_work, uint8_t *d_pred, uint32_t *d_age, uint32_t *d_id,
                               uint32_t *d_len, uint32_t *d_track, uint8_t *d_flags_out, void *stream);

/*
 * The same for a batch in HOST memory: copies the inputs to the device, runs the call above with a workspace of its own,
 * copies the outputs back; synchronous.  `list` needs no alignment here.  MT_ERR_INVALID also for decreasing stream_off
 * and for stream_off[n_streams] > n_frames.
 */
int mtgpu_track_objects(mtgpu_ctx *ctx, const uint8_t *flags, const uint8_t *has_sd, const struct mt_object *list, int32_t k,
                        uint32_t n_frames, const uint64_t *stream_off, uint32_t n_streams, uint32_t min_cells,
                        uint32_t max_dropout, uint32_t reach, uint32_t min_track, uint8_t *pred, uint32_t *age, uint32_t *id,
                        uint32_t *len, uint32_t *track, uint8_t *flags_out);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_TRACKS_H */
