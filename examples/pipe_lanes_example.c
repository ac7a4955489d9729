/* pipe_lanes_example.c — a direction plane on the decode path: lanes_example.c's recording — a camera over a two-way road
 * on a 12 x 8 grid, a car driving EAST in the upper half (the far lane, where traffic goes west) through frames 10 .. 19
 * and another driving east in the lower half through frames 40 .. 49 — fed frame by frame through a pipe, as a decode
 * loop feeds it (decoder -> mtgpu_batch_add_frame -> mtgpu_pipe_submit -> flags -> merge).  mtgpu_pipe_set_dir has one
 * byte for the whole picture and cannot tell the two cars apart; mtgpu_pipe_set_plane gives every cell its own byte.
 * Under 0xFF bytes the pipe keeps 20 frames in 2 segments, under the plane 10 in 1.
 *
 *   gcc -std=c11 -Iinclude examples/pipe_lanes_example.c -o pipe_lanes_example \
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

enum { F = 60, GW = 12, GH = 8 };

static double g_ts[F];
static uint64_t g_kept = 0;
static int g_inflight = 0;

/* wait for the oldest batch, keep the timestamps of its motion frames (:382-383), free the batch */
static int collect(mtgpu_pipe *pipe) {
  mtgpu_batch *b = NULL;
  const uint8_t *flags = NULL;
  const double *pts = NULL;
  uint32_t n = 0;
  CHECK(mtgpu_pipe_collect(pipe, &b, &flags, &pts, NULL, &n));
  for (uint32_t i = 0; i < n; ++i)
    if (flags[i]) g_ts[g_kept++] = pts[i];
  --g_inflight;
  CHECK(mtgpu_pipe_release(pipe, b));
  return 0;
}

static void add_cell(mt_mv *mv, size_t *n, int gx, int gy, int dx, int dy) {
  for (int k = 0; k < 2; ++k) {                  /* two votes per cell (VECTORS_NEEDED 2) */
    mt_mv *v = &mv[(*n)++];
    v->dst_x = (int16_t)(16 * gx + 8);
    v->dst_y = (int16_t)(16 * gy + 8);
    v->src_x = (int16_t)(v->dst_x - dx);
    v->src_y = (int16_t)(v->dst_y - dy);
  }
}

/* the decode loop, then the merge on the frames it kept */
static int scan(mtgpu_ctx *ctx, mtgpu_pipe *pipe, const char *label, uint64_t *kept, uint64_t *segments) {
  static mt_mv side_data[16];                    /* stands for the AVFrame's side data */
  mtgpu_batch *cur = NULL;
  g_kept = 0;
  for (int f = 0; f < F; ++f) {
    size_t n = 0;
    memset(side_data, 0, sizeof side_data);
    if (f >= 10 && f < 20)
      for (int c = 0; c < 3; ++c) add_cell(side_data, &n, 2 + (f - 10) / 2 + c, 2, 6, 0);   /* the car in the far lane */
    if (f >= 40 && f < 50)
      for (int c = 0; c < 3; ++c) add_cell(side_data, &n, 2 + (f - 40) / 2 + c, 5, 6, 0);   /* the car in the near lane */
    for (;;) {
      if (!cur) {
        int rc = mtgpu_pipe_acquire(pipe, &cur);
        if (rc == MT_ERR_BUSY) { if (collect(pipe)) return 1; continue; }   /* back-pressure */
        CHECK(rc);
      }
      int rc = mtgpu_batch_add_frame(cur, side_data, n * sizeof(mt_mv), 1, f / 25.0, (uint64_t)f);
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
  const mt_merge_params mp = {0.2, 0.04, F / 25.0, 5.0};
  mt_segment seg[8];
  mt_merge_result res;
  CHECK(mtgpu_merge_segments(ctx, g_ts, g_kept, &mp, 0, seg, 8, &res));
  *kept = g_kept;
  *segments = res.n_segments;
  printf("%-28s %2llu frames kept, %llu segment(s)", label, (unsigned long long)g_kept, (unsigned long long)res.n_segments);
  for (uint64_t s = 0; s < res.n_segments && s < 8; ++s) printf("  [%.2f, %.2f]", seg[s].start, seg[s].end);
  printf("\n");
  return 0;
}

int main(void) {
  /* 192 x 128 pixels in 16-pixel blocks: 12 x 8 cells; reference code defaults but no vertical mask */
  mt_scan_params p;
  CHECK(mtgpu_params_from_config(&p, 16 * GW, 16 * GH, 16.0, 16, 4, 2, 2, 0.0f));
  if (p.grid_w != GW || p.grid_h != GH) {
    fprintf(stderr, "unexpected grid %d x %d\n", p.grid_w, p.grid_h);
    return 1;
  }
  mtgpu_ctx *ctx = NULL;
  CHECK(mtgpu_create(&p, 0, &ctx));
  mtgpu_pipe *pipe = NULL;
  CHECK(mtgpu_pipe_create_layout(ctx, 256, 16, 3, MT_LAYOUT_COMPACT8 | MT_LAYOUT_ZERO_COPY, &pipe));

  /* sectors clockwise from E: E 0, SE 1, S 2, SW 3, W 4, NW 5, N 6, NE 7.  plane[y * GW + x]: the byte of cell (x, y) */
  uint8_t everything[GW * GH], plane[GW * GH], back[GW * GH];
  memset(everything, MTGPU_DIR_ALL, sizeof everything);
  for (int y = 0; y < GH; ++y)
    for (int x = 0; x < GW; ++x) plane[y * GW + x] = y < GH / 2 ? (uint8_t)(MTGPU_DIR_ALL & ~(1 << 0 | 1 << 7 | 1 << 1)) : MTGPU_DIR_ALL;

  uint64_t kept_all, seg_all, kept_plane, seg_plane;
  if (mtgpu_pipe_plane(pipe, NULL, NULL) != 0) return 2;
  CHECK(mtgpu_pipe_set_plane(pipe, everything, MT_PIPE_REPORT_CENTRES));
  if (scan(ctx, pipe, "0xFF everywhere", &kept_all, &seg_all)) return 1;
  CHECK(mtgpu_pipe_set_plane(pipe, plane, MT_PIPE_REPORT_CENTRES));
  int report = -1;
  if (mtgpu_pipe_plane(pipe, back, &report) != 1 || memcmp(back, plane, sizeof plane) || report != MT_PIPE_REPORT_CENTRES) return 2;
  if (scan(ctx, pipe, "upper half: not E, NE, SE", &kept_plane, &seg_plane)) return 1;

  CHECK(mtgpu_pipe_set_plane(pipe, NULL, 0));     /* the next recording: the plain scan, as before */
  if (mtgpu_pipe_plane(pipe, NULL, NULL) != 0) return 2;
  mtgpu_pipe_destroy(pipe);
  mtgpu_destroy(ctx);
  if (!(kept_all == 20 && seg_all == 2 && kept_plane == 10 && seg_plane == 1)) {
    fprintf(stderr, "unexpected counts\n");
    return 3;
  }
  return 0;
}
