/* pipe_zones_example.c — pipe_example.c with an ignore zone: the decode loop of src/motion_scanner.cpp:375-383 feeds a
 * pipe that carries a keep mask (mtgpu_pipe_set_keep, include/mtgpu_pipe_zones.h), so the cells of the zone never count
 * (:282 with one more term) and the segments are cut accordingly.  The recording is scanned twice through ONE pipe:
 * under the mask, then — mtgpu_pipe_set_keep(pipe, NULL) — without it.  Plain C against include/mtgpu.h.
 *
 *   gcc -std=c11 -Iinclude examples/pipe_zones_example.c -o pipe_zones_example \
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

/* the decode loop: motion in seconds 2-3 at cells (40..41, 30) and in seconds 8-9 at cells (100..101, 30) */
static int scan(mtgpu_pipe *pipe) {
  enum { F = 300, PER = 4 };
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
        v->dst_x = (int16_t)(16 * ((first ? 40 : 100) + k / 2) + 8);
        v->dst_y = (int16_t)(16 * 30 + 8);
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
  CHECK(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 2, 2, 0.05f));
  mtgpu_ctx *ctx = NULL;
  CHECK(mtgpu_create(&p, 0, &ctx));
  mtgpu_pipe *pipe = NULL;
  CHECK(mtgpu_pipe_create(ctx, 4096, 16, 3, &pipe));

  /* the keep mask: everything is analysed but the road at the right, columns 96.. of every row */
  mtgpu_zones_plan zp;
  CHECK(mtgpu_zones_preview(&p, 163840, &zp));
  uint64_t *keep = malloc(sizeof(uint64_t) * (size_t)zp.keep_words_per_stream);
  if (!keep) return 1;
  for (int y = 0; y < p.grid_h; ++y)
    for (int w = 0; w < zp.keep_words_per_row; ++w) {
      uint64_t word = 0;
      for (int b = 0; b < 64; ++b) {
        const int x = w * 64 + b;
        if (x < p.grid_w && x < 96) word |= (uint64_t)1 << b;
      }
      keep[(size_t)y * (size_t)zp.keep_words_per_row + (size_t)w] = word;
    }
  CHECK(mtgpu_pipe_set_keep(pipe, keep));          /* copied: the buffer is ours again */
  free(keep);
  if (mtgpu_pipe_has_keep(pipe) != 1) return 2;

  mt_merge_params mp = {5.0, 0.5, 300 / 30.0, 5.0};   /* MAX_GAP_SEC, PADDING_SEC, duration, MIN_SAVINGS_PCT */
  mt_segment seg[8];
  mt_merge_result r;
  if (scan(pipe)) return 1;
  const size_t masked_frames = g_nts;
  CHECK(mtgpu_merge_segments(ctx, g_ts, g_nts, &mp, 1, seg, 8, &r));
  const uint64_t masked_segments = r.n_segments;
  printf("with the zone:    motion frames %zu, segments %llu\n", g_nts, (unsigned long long)r.n_segments);
  for (uint64_t i = 0; i < r.n_segments; ++i) printf("  [%.3f, %.3f]\n", seg[i].start, seg[i].end);

  CHECK(mtgpu_pipe_set_keep(pipe, NULL));          /* the next recording has no zones: the plain scan again */
  if (mtgpu_pipe_has_keep(pipe) != 0) return 2;
  if (scan(pipe)) return 1;
  CHECK(mtgpu_merge_segments(ctx, g_ts, g_nts, &mp, 1, seg, 8, &r));
  printf("without the zone: motion frames %zu, segments %llu\n", g_nts, (unsigned long long)r.n_segments);
  for (uint64_t i = 0; i < r.n_segments; ++i) printf("  [%.3f, %.3f]\n", seg[i].start, seg[i].end);
  mtgpu_pipe_destroy(pipe);
  mtgpu_destroy(ctx);
  /* frames 60 and 240 are keyframes: 29 motion frames per burst; the zone removes the second burst */
  return (masked_frames == 29 && masked_segments == 1 && g_nts == 58 && r.n_segments == 2) ? 0 : 3;
}
