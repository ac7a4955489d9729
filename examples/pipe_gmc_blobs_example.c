/*
 * pipe_gmc_blobs_example.c — the compensated blob scan on the decode path, plain C (include/mtgpu_pipe_gmc_blobs.h).
 *
 * A shaking camera in the rain: the whole picture moves by a few pixels in every frame, and in every frame a few
 * scattered pairs of cells move on their own (drops on the lens, noise of the encoder's search).  In one second an
 * object of 4 x 2 cells crosses the picture.
 *   plain scan          keeps every frame: the pan passes the threshold everywhere.
 *   mtgpu_pipe_set_gmc  keeps every frame: after the pan is subtracted the scattered pairs still give 8 centres, and
 *                       CLUSTERS_NEEDED cannot tell them from an object.
 *   mtgpu_pipe_set_blobs(3)   keeps every frame: the whole panned region is one blob of 2360 cells.
 *   mtgpu_pipe_set_gmc_blobs(3)   keeps the second with the object: the largest blob of the RESIDUAL vote is 2 cells in
 *                       the rain and 8 cells with the object.
 *
 *   cc -std=c11 -Iinclude examples/pipe_gmc_blobs_example.c -L<package dir> -lmtgpu -Wl,-rpath,<package dir> -o pipe_gmc_blobs_example
 */
#include <stdio.h>
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

static size_t g_motion = 0;
static int g_inflight = 0;

/* wait for the oldest batch, count its motion frames (:382-383), free the batch */
static int collect(mtgpu_pipe *pipe) {
  mtgpu_batch *b = NULL;
  const uint8_t *flags = NULL;
  uint32_t n = 0;
  CHECK(mtgpu_pipe_collect(pipe, &b, &flags, NULL, NULL, &n));
  for (uint32_t i = 0; i < n; ++i)
    if (flags[i]) ++g_motion;
  --g_inflight;
  CHECK(mtgpu_pipe_release(pipe, b));
  return 0;
}

/* the decode loop: 10 seconds at 30 frames/s.  Every frame carries the shaking background on rows 20 .. 39 (two records
 * per cell, VECTORS_NEEDED 2), moving by the frame's pan.  Four pairs of cells, on rows 22, 29, 33 and 37 and at columns
 * that change from frame to frame, move 5 pixels faster than the pan: the rain.  In seconds 4-5 an object of 4 x 2 cells
 * at (50 .. 53, 25 .. 26) moves 6 pixels faster than the pan. */
static int scan(mtgpu_pipe *pipe) {
  enum { F = 300, ROWS = 20, BG = 120 * ROWS, MAXREC = 2 * BG };
  static const int rain_row[4] = {22, 29, 33, 37};
  static mt_mv side_data[MAXREC];                  /* stands for the AVFrame's side data */
  mtgpu_batch *cur = NULL;
  g_motion = 0;
  for (int f = 0; f < F; ++f) {
    const int pan_x = 5 + f % 5, pan_y = -(2 + f % 3);   /* never (0, 0), always above the threshold: 25 + 4 >= 16 */
    const int object = f >= 120 && f < 150;
    size_t n = 0;
    memset(side_data, 0, sizeof side_data);
    for (int c = 0; c < BG; ++c) {
      const int gx = c % 120, gy = 20 + c / 120;
      int extra = 0;
      for (int i = 0; i < 4; ++i) {
        const int x0 = 3 + (f * 7 + i * 29) % 110;
        if (gy == rain_row[i] && (gx == x0 || gx == x0 + 1)) extra = 5;
      }
      if (object && gx >= 50 && gx < 54 && gy >= 25 && gy < 27) extra = 6;
      for (int k = 0; k < 2; ++k) {
        mt_mv *v = &side_data[n++];
        v->dst_x = (int16_t)(16 * gx + 8);
        v->dst_y = (int16_t)(16 * gy + 8);
        v->src_x = (int16_t)(v->dst_x - (pan_x + extra));
        v->src_y = (int16_t)(v->dst_y - pan_y);
      }
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
  CHECK(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 2, 2, 0.05f));   /* the defaults: VECTORS_NEEDED 2, CLUSTERS_NEEDED 2 */
  mtgpu_ctx *ctx = NULL;
  CHECK(mtgpu_create(&p, 0, &ctx));
  mtgpu_pipe *pipe = NULL;
  CHECK(mtgpu_pipe_create(ctx, 16 * 4800, 16, 3, &pipe));

  size_t frames[4];
  if (mtgpu_pipe_gmc_blobs(pipe, NULL, NULL, NULL, NULL) != 0) return 2;
  if (scan(pipe)) return 1;
  frames[0] = g_motion;
  printf("plain scan:                          motion frames %zu\n", g_motion);

  CHECK(mtgpu_pipe_set_gmc(pipe, 1, MTGPU_GMC_DEFAULT_MAX_SHIFT, MTGPU_GMC_DEFAULT_MIN_SHARE_Q8, MT_PIPE_REPORT_CENTRES));
  if (scan(pipe)) return 1;
  frames[1] = g_motion;
  printf("compensated (set_gmc):               motion frames %zu  (the rain leaves 8 centres)\n", g_motion);
  CHECK(mtgpu_pipe_set_gmc(pipe, 0, 0, 0, 0));

  CHECK(mtgpu_pipe_set_blobs(pipe, 3, MT_PIPE_REPORT_CENTRES));
  if (scan(pipe)) return 1;
  frames[2] = g_motion;
  printf("blobs of 3 cells (set_blobs):        motion frames %zu  (the pan is one blob)\n", g_motion);
  /* the pair is a mode of its own: while a single mode is on it is refused, and the pipe stays as it is */
  if (mtgpu_pipe_set_gmc_blobs(pipe, 3, MTGPU_GMC_DEFAULT_MAX_SHIFT, MTGPU_GMC_DEFAULT_MIN_SHARE_Q8, MT_PIPE_REPORT_CENTRES) != MT_ERR_INVALID)
    return 2;
  CHECK(mtgpu_pipe_set_blobs(pipe, 0, 0));

  CHECK(mtgpu_pipe_set_gmc_blobs(pipe, 3, MTGPU_GMC_DEFAULT_MAX_SHIFT, MTGPU_GMC_DEFAULT_MIN_SHARE_Q8, MT_PIPE_REPORT_CENTRES));
  int32_t cells = -1, ms = -1, q8 = -1;
  int report = -1;
  if (mtgpu_pipe_gmc_blobs(pipe, &cells, &ms, &q8, &report) != 1 || cells != 3 || ms != 16 || q8 != 128 || report != MT_PIPE_REPORT_CENTRES)
    return 2;
  if (mtgpu_pipe_gmc(pipe, NULL, NULL, NULL) != 0 || mtgpu_pipe_blobs(pipe, NULL, NULL) != 0) return 2;
  if (scan(pipe)) return 1;
  frames[3] = g_motion;
  printf("compensated blobs (set_gmc_blobs):   motion frames %zu\n", g_motion);

  CHECK(mtgpu_pipe_set_gmc_blobs(pipe, 0, 0, 0, 0));   /* the next recording: the plain pipe, as before */
  mtgpu_pipe_destroy(pipe);
  mtgpu_destroy(ctx);
  /* 10 keyframes carry no side data: 290 frames move; frame 120 is a keyframe: the object shows in 29 frames */
  return (frames[0] == 290 && frames[1] == 290 && frames[2] == 290 && frames[3] == 29) ? 0 : 3;
}
