/* pipe_blobs_example.c — pipe_example.c with a minimum object size: the decode loop of src/motion_scanner.cpp:375-383
 * feeds a pipe that runs the blob scan (mtgpu_pipe_set_blobs, include/mtgpu_pipe_blobs.h), so a frame counts only when
 * the largest 4-connected blob of its centre cells (:272-294) has at least MIN_BLOB_CELLS cells.  The recording is
 * scanned three times through ONE pipe: plainly, under the rule, then — mtgpu_pipe_set_blobs(pipe, 0, 0) — plainly
 * again.  Plain C against include/mtgpu.h.
 *
 *   gcc -std=c11 -Iinclude examples/pipe_blobs_example.c -o pipe_blobs_example \
 *       -Lmotion-estimated-video-trimmer_amd -lmtgpu -Wl,-rpath,$PWD/motion-estimated-video-trimmer_amd
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mtgpu.h"

#define CHECK(call)                                                        \
  do {                                                                     \
    int rc_ = (call);                                                      \
    if (rc_ != MT_OK) {                                                    \
      fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mtgpu_last_error());   \
      return 1;                                                            \
    }                                                                      \
  } while (0)

static double g_ts[4096];
static size_t g_nts = 0;
static int g_inflight = 0;

/* wait for the oldest batch, keep the timestamps of its motion frames (:382-383), free the batch */
static int collect(mtgpu_pipe *pipe) {
  mtgpu_batch *b = NULL;
  const uint8_t *flags = NULL;
  const double *pts = NULL;
  uint32_t n = 0;
  CHECK(mtgpu_pipe_collect(pipe, &b, &flags, &pts, NULL, &n));
  for (uint32_t i = 0; i < n; ++i)
    if (flags[i]) g_ts[g_nts++] = pts[i];
  --g_inflight;
  CHECK(mtgpu_pipe_release(pipe, b));
  return 0;
}

/* the decode loop: rain in seconds 2-3 — four separate pairs of cells, 8 centres in 4 blobs of 2 — and one object in
 * seconds 8-9 — a block of 4 x 2 cells, 8 centres in 1 blob of 8 */
static int scan(mtgpu_pipe *pipe) {
  enum { F = 300, PER = 8 };
  static const int rain[PER][2] = {{10, 10}, {11, 10}, {30, 20}, {31, 20}, {70, 40}, {71, 40}, {100, 55}, {101, 55}};
  mtgpu_batch *cur = NULL;
  g_nts = 0;
  for (int f = 0; f < F; ++f) {
    mt_mv side_data[PER];                          /* stands for the AVFrame's side data: dies with the frame (:347) */
    size_t n = 0;
    const int first = f >= 60 && f < 90, second = f >= 240 && f < 270;
    memset(side_data, 0, sizeof side_data);
    if (first || second)
      for (int k = 0; k < PER; ++k) {
        mt_mv *v = &side_data[n++];
        const int gx = first ? rain[k][0] : 40 + k % 4, gy = first ? rain[k][1] : 30 + k / 4;
        v->dst_x = (int16_t)(16 * gx + 8);
        v->dst_y = (int16_t)(16 * gy + 8);
        v->src_x = (int16_t)(v->dst_x - 6);
        v->src_y = v->dst_y;
      }
    const int is_keyframe = (f % 30) == 0;         /* I-frames export no MV side data (:219-221) */
    for (;;) {
      if (!cur) {
        int rc = mtgpu_pipe_acquire(pipe, &cur);
        if (rc == MT_ERR_BUSY) { if (collect(pipe)) return 1; continue; }   /* back-pressure */
        CHECK(rc);
      }
      int rc = mtgpu_batch_add_frame(cur, is_keyframe ? NULL : side_data, n * sizeof(mt_mv), !is_keyframe, f / 30.0,
                                     (uint64_t)f);
      if (rc == MT_ERR_CAPACITY) {                 /* batch full: ship it, start the next one */
        CHECK(mtgpu_pipe_submit(pipe, cur));
        cur = NULL;
        ++g_inflight;
        continue;
      }
      CHECK(rc);
      break;
    }
  }
  if (cur) { CHECK(mtgpu_pipe_submit(pipe, cur)); ++g_inflight; }
  while (g_inflight > 0)
    if (collect(pipe)) return 1;
  return 0;
}

int main(void) {
  mt_scan_params p;
  CHECK(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 1, 8, 0.05f));   /* VECTORS_NEEDED 1, CLUSTERS_NEEDED 8 */
  mtgpu_ctx *ctx = NULL;
  CHECK(mtgpu_create(&p, 0, &ctx));
  mtgpu_pipe *pipe = NULL;
  CHECK(mtgpu_pipe_create(ctx, 4096, 16, 3, &pipe));

  mt_merge_params mp = {5.0, 0.5, 300 / 30.0, 5.0};   /* MAX_GAP_SEC, PADDING_SEC, duration, MIN_SAVINGS_PCT */
  mt_segment seg[8];
  mt_merge_result r;
  int32_t n = -1;
  int report = -1;

  /* CLUSTERS_NEEDED alone keeps the rain: it cannot tell four pairs from one object of eight cells */
  if (mtgpu_pipe_blobs(pipe, &n, &report) != 0) return 2;
  if (scan(pipe)) return 1;
  const size_t plain_frames = g_nts;
  CHECK(mtgpu_merge_segments(ctx, g_ts, g_nts, &mp, 1, seg, 8, &r));
  const uint64_t plain_segments = r.n_segments;
  printf("CLUSTERS_NEEDED 8 alone:  motion frames %zu, segments %llu\n", g_nts, (unsigned long long)r.n_segments);
  for (uint64_t i = 0; i < r.n_segments; ++i) printf("  [%.3f, %.3f]\n", seg[i].start, seg[i].end);

  /* a minimum object size of 3 cells: every batch of the pipe now runs the blob scan */
  CHECK(mtgpu_pipe_set_blobs(pipe, 3, MT_PIPE_REPORT_CENTRES));
  if (mtgpu_pipe_blobs(pipe, &n, &report) != 1 || n != 3 || report != MT_PIPE_REPORT_CENTRES) return 2;
  if (scan(pipe)) return 1;
  const size_t blob_frames = g_nts;
  CHECK(mtgpu_merge_segments(ctx, g_ts, g_nts, &mp, 1, seg, 8, &r));
  const uint64_t blob_segments = r.n_segments;
  printf("with MIN_BLOB_CELLS 3:    motion frames %zu, segments %llu\n", g_nts, (unsigned long long)r.n_segments);
  for (uint64_t i = 0; i < r.n_segments; ++i) printf("  [%.3f, %.3f]\n", seg[i].start, seg[i].end);

  CHECK(mtgpu_pipe_set_blobs(pipe, 0, 0));         /* the next recording has no such rule: the plain scan again */
  if (mtgpu_pipe_blobs(pipe, NULL, NULL) != 0) return 2;
  if (scan(pipe)) return 1;
  mtgpu_pipe_destroy(pipe);
  mtgpu_destroy(ctx);
  /* frames 60 and 240 are keyframes: 29 motion frames per burst; the rule removes the rain */
  return (plain_frames == 58 && plain_segments == 2 && blob_frames == 29 && blob_segments == 1 && g_nts == 58) ? 0 : 3;
}
