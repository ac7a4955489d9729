/*
 * mtgpu_sweep.h — one scan of the records for a whole grid of (MV_THRESHOLD_SQ, VECTORS_NEEDED) settings: part of the
 * C ABI of mtgpu.h, which includes this header (include either one).  Same conventions: MT_* status codes, arguments
 * validated before anything is launched, the `*_device` entry point takes device pointers (or driver-allocated pinned
 * host memory through its device address) and is asynchronous on `stream`, the other takes host pointers and is
 * synchronous; NO CPU fallback; no environment variables.
 *
 * What is computed: for every threshold t and vector level v of the call, the centre count of every frame — the
 * `clusters` counter of src/motion_scanner.cpp:272-294 without its early return — that a scanner configured with
 * MV_THRESHOLD_SQ = thresholds[t] and VECTORS_NEEDED = vectors[v] would count; exactly what mtgpu_scan_centres_device
 * returns through a context created with that pair.  The thresholds are nested (:251 keeps a record iff
 * !(|d|^2 < T), so a record that passes T passes every smaller one) and a cell's vote count answers every
 * VECTORS_NEEDED (:282), so the records are read once for all settings that fit LDS together; the per-setting work is
 * the cluster test over the LDS-resident grid.  mtgpu_sweep_streams_device then turns each setting's counts into
 * segments for every CLUSTERS_NEEDED: the whole three-dimensional sensitivity study.
 *
 * From the context only the grid, block_shift and vertical margin are used; its own mv_threshold_sq, vectors_needed
 * and clusters_needed play no part.
 *
 *   thresholds   HOST array of n_thresholds doubles in [1, MT_SWEEP_MAX_THRESHOLDS], copied at call time, any order,
 *                duplicates allowed; each follows MV_THRESHOLD_SQ exactly (:251): NaN or <= 0 keeps every record,
 *                +inf keeps none
 *   vectors      HOST array of n_vectors levels in [1, MT_SWEEP_MAX_VECTORS], copied at call time, any order, duplicates
 *                allowed; each is wrapped to uint8 as mtgpu_params_from_config wraps VECTORS_NEEDED (:186, config.hpp:75);
 *                level 0 makes every cell of the grid active
 *   d_centres    n_thresholds * n_vectors * n_frames uint32, setting-major in the CALLER's order:
 *                d_centres[(t * n_vectors + v) * n_frames + f].  One setting's slice is what
 *                mtgpu_flags_from_centres_device and mtgpu_sweep_streams_device take.  Every element is written: 0 for
 *                a frame without side data (:219-221).
 *
 * Kernel (csrc/sweep_kernels.hip): one workgroup per frame with side data, 32-bit LDS counters, one tile of
 * (analysed rows + 2) x grid_w counters per threshold.  When the tiles of all thresholds do not fit LDS together the
 * call runs several launches, each over a contiguous run of the sorted thresholds, and EVERY launch reads the records
 * again: bytes read = passes x the batch (mtgpu_scan_sweep_preview tells `passes`).  A grid for which not even one
 * tile and a three-row mask buffer fit (960x540 cells, 32767-wide grids: the grids the plain scan cuts into row
 * bands) is MT_ERR_UNSUPPORTED.  One workgroup per frame, no slicing of large frames and no grouping of small ones: a
 * launch of a few frames, or of very small frames, does not fill the chip.
 */
#ifndef MTGPU_SWEEP_H
#define MTGPU_SWEEP_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MT_SWEEP_MAX_THRESHOLDS 8
#define MT_SWEEP_MAX_VECTORS 8

/* How a sweep of n_thresholds x n_vectors settings runs on a grid. */
typedef struct mtgpu_sweep_plan {
  int32_t thresholds_per_pass; /* tiles resident in LDS per launch                          */
  int32_t passes;              /* launches = reads of the records: ceil(n_thresholds / fit) */
  int32_t lds_bytes;           /* dynamic LDS per workgroup                                 */
  int32_t counter_bits;        /* 32                                                        */
} mtgpu_sweep_plan;

/*
 * The plan mtgpu_scan_sweep_device would pick for these parameters on a device with `lds_bytes_per_workgroup` of LDS
 * per workgroup (MI355X: 163840).  Pure host arithmetic: no HIP call, works without a device.  Of `p` only the grid
 * and the vertical margin matter (the analysed rows of src/motion_scanner.cpp:237-238 size a tile).
 * MT_ERR_INVALID: n_thresholds / n_vectors outside their ranges, invalid parameters; MT_ERR_UNSUPPORTED: not even one
 * tile fits.  thresholds_per_pass * passes >= n_thresholds.
 */
int mtgpu_scan_sweep_preview(const mt_scan_params *p, int lds_bytes_per_workgroup, uint32_t n_thresholds,
                             uint32_t n_vectors, mtgpu_sweep_plan *out);

/*
 * The centre counts (src/motion_scanner.cpp:272-294) of every setting for a device-resident batch; asynchronous on
 * `stream`.  d_rec / rec_bytes / n_records / d_frame_off / d_has_sd / n_frames as for mtgpu_scan_centres_device
 * (rec_bytes 40 = mt_mv, 8 = mt_mv_compact, 8-byte aligned).  thresholds, vectors, d_centres: see above.
 * n_frames == 0: MT_OK, nothing is written.  MT_ERR_INVALID (the argument is named in mtgpu_last_error) for rec_bytes
 * outside {8, 40}, a misaligned pointer, NULL thresholds / vectors / d_centres / d_frame_off and counts outside their
 * ranges; MT_ERR_UNSUPPORTED (the grid is named) for a grid without a single-tile form.  Nothing is launched and no
 * output word is touched when the call fails this way.  d_centres in pinned host memory is written with system-scope
 * stores, as mtgpu_scan_centres_device writes its counts.  Launch scratch (32 bytes per frame) comes from the
 * context's ring; with mtgpu_profile_enable on, the call records the same event triple as a scan launch
 * (all passes count as scan time).
 */
int mtgpu_scan_sweep_device(mtgpu_ctx *ctx, const void *d_rec, int rec_bytes, uint64_t n_records,
                            const uint64_t *d_frame_off, const uint8_t *d_has_sd /* may be NULL */, uint32_t n_frames,
                            const double *thresholds, uint32_t n_thresholds, const int32_t *vectors, uint32_t n_vectors,
                            uint32_t *d_centres, void *stream);

/*
 * The same for a batch in HOST memory (src/motion_scanner.cpp:217-295 for every frame and setting): copies the
 * records the offsets span, the offsets and has_sd to the device, runs the sweep, copies the counts back;
 * synchronous.  mv / frame_off / has_sd / n_frames as for mtgpu_scan_frames_centres; centres:
 * n_thresholds * n_vectors * n_frames uint32, laid out as d_centres above.  MT_ERR_INVALID also for decreasing offsets.
 */
int mtgpu_scan_frames_sweep(mtgpu_ctx *ctx, const mt_mv *mv, const uint64_t *frame_off,
                            const uint8_t *has_sd /* may be NULL */, uint32_t n_frames, const double *thresholds,
                            uint32_t n_thresholds, const int32_t *vectors, uint32_t n_vectors, uint32_t *centres);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_SWEEP_H */
