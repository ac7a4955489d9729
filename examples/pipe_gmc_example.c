/*
 * pipe_gmc_example.c — global-motion compensation on the decode path, plain C (include/mtgpu_pipe_gmc.h).
 *
 * A camera on a pole in wind: the whole picture moves by a few pixels in every frame, and a clock is burnt into the top
 * left corner.  The plain scan keeps every frame.  Compensation alone still keeps every frame: the clock does not move
 * with the picture, so its residual is minus the pan.  Compensation under a keep mask that ignores the clock keeps only
 * the second in which something crosses the picture.
 *
 *   cc -std=c11 -Iinclude examples/pipe_gmc_example.c -L<package dir> -lmtgpu -Wl,-rpath,<package dir> -o pipe_gmc_example
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

/* the decode loop: 10 seconds at 30 frames/s.  Every frame carries the shaking background on rows 20 .. 23 (two records
 * per cell, VECTORS_NEEDED 2), moving by the frame's pan, and the still clock on cells (5 .. 14, 6 .. 8).  In seconds 4-5
 * an object of 2 x 2 cells moves 6 pixels faster than the pan. */
static int scan(mtgpu_pipe *pipe) {
  enum { F = 300, BG = 120 * 4, CLOCK = 10 * 3, MAXREC = 2 * (BG + CLOCK) };
  static mt_mv side_data[MAXREC];                  /* stands for the AVFrame's side data */
  mtgpu_batch *cur = NULL;
  g_nts = 0;
  for (int f = 0; f < F; ++f) {
    const int pan_x = 5 + f % 5, pan_y = -(2 + f % 3);   /* never (0, 0), always above the threshold: 25 + 4 >= 16 */
    const int object = f >= 120 && f < 150;
    size_t n = 0;
    memset(side_data, 0, sizeof side_data);
    for (int c = 0; c < BG + CLOCK; ++c) {
      const int clock = c >= BG;
      const int gx = clock ? 5 + (c - BG) % 10 : c % 120, gy = clock ? 6 + (c - BG) / 10 : 20 + c / 120;
      const int fast = object && !clock && gx >= 50 && gx < 52 && gy >= 21 && gy < 23;
      for (int k = 0; k < 2; ++k) {
        mt_mv *v = &side_data[n++];
        v->dst_x = (int16_t)(16 * gx + 8);
        v->dst_y = (int16_t)(16 * gy + 8);
        v->src_x = (int16_t)(v->dst_x - (clock ? 0 : pan_x + (fast ? 6 : 0)));
        v->src_y = (int16_t)(v->dst_y - (clock ? 0 : pan_y));
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
  CHECK(mtgpu_pipe_create(ctx, 16384, 16, 3, &pipe));

  /* the keep plane: 68 rows of two 64-bit words, every cell kept but the clock's */
  static uint64_t keep[68 * 2];
  for (int i = 0; i < 68 * 2; ++i) keep[i] = ~0ull;
  for (int y = 6; y < 9; ++y)
    for (int x = 5; x < 15; ++x) keep[y * 2 + (x >> 6)] &= ~(1ull << (x & 63));

  size_t frames[4];
  if (mtgpu_pipe_gmc(pipe, NULL, NULL, NULL) != 0) return 2;
  if (scan(pipe)) return 1;
  frames[0] = g_nts;
  printf("plain scan:                       motion frames %zu\n", g_nts);

  CHECK(mtgpu_pipe_set_gmc(pipe, 1, MTGPU_GMC_DEFAULT_MAX_SHIFT, MTGPU_GMC_DEFAULT_MIN_SHARE_Q8, MT_PIPE_REPORT_CENTRES));
  int32_t ms = -1, q8 = -1;
  int report = -1;
  if (mtgpu_pipe_gmc(pipe, &ms, &q8, &report) != 1 || ms != 16 || q8 != 128 || report != MT_PIPE_REPORT_CENTRES) return 2;
  if (scan(pipe)) return 1;
  frames[1] = g_nts;
  printf("compensated, no mask:             motion frames %zu  (the clock's residual is minus the pan)\n", g_nts);

  CHECK(mtgpu_pipe_set_keep(pipe, keep));
  if (scan(pipe)) return 1;
  frames[2] = g_nts;
  printf("compensated, the clock ignored:   motion frames %zu\n", g_nts);
  mt_merge_params mp = {5.0, 0.5, 300 / 30.0, 5.0};   /* MAX_GAP_SEC, PADDING_SEC, duration, MIN_SAVINGS_PCT */
  mt_segment seg[8];
  mt_merge_result r;
  CHECK(mtgpu_merge_segments(ctx, g_ts, g_nts, &mp, 1, seg, 8, &r));
  for (uint64_t i = 0; i < r.n_segments; ++i) printf("  [%.3f, %.3f]\n", seg[i].start, seg[i].end);

  CHECK(mtgpu_pipe_set_gmc(pipe, 0, 0, 0, 0));     /* the next recording: the masked scan alone, as before */
  if (mtgpu_pipe_gmc(pipe, NULL, NULL, NULL) != 0 || mtgpu_pipe_has_keep(pipe) != 1) return 2;
  if (scan(pipe)) return 1;
  frames[3] = g_nts;
  mtgpu_pipe_destroy(pipe);
  mtgpu_destroy(ctx);
  /* 10 keyframes carry no side data: 290 frames move; frame 120 is a keyframe: the object shows in 29 frames */
  return (frames[0] == 290 && frames[1] == 290 && frames[2] == 29 && r.n_segments == 1 && frames[3] == 290) ? 0 : 3;
}
