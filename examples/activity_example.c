/* activity_example.c — WHERE a stream moves: the per-cell activity map of two tiny streams (for every grid cell, the
 * frames in which it was active and the frames in which it was one of the centres src/motion_scanner.cpp:277-292
 * counts), once over every frame with side data and once over the frames the trimmer would keep.
 *
 *   gcc -std=c11 -Iinclude examples/activity_example.c -o activity_example \
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

int main(void) {
  /* 1080p, reference code defaults, but no vertical mask: the map is what a mask is chosen on */
  mt_scan_params p;
  CHECK(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 2, 2, 0.0f));
  mtgpu_ctx *ctx = NULL;
  CHECK(mtgpu_create(&p, 0, &ctx));
  mtgpu_activity_plan plan;
  CHECK(mtgpu_activity_preview(&p, 163840, &plan));
  printf("plan: %d bytes of LDS, %d-bit accumulators, runs of up to %d frames\n", plan.lds_bytes, plan.acc_bits, plan.max_run);

  /* Two streams of 30 frames.  Stream 0: a clock in the top row (cells (100..102, 0)) ticks in every frame, an object
   * (cells (40..43, 30)) passes in frames 10..19.  Stream 1: only the clock, and only two cells of it. */
  enum { S = 2, F = 60, MAX_CELLS = 7 };
  mt_mv *mv = calloc((size_t)F * MAX_CELLS * 2, sizeof *mv);
  uint64_t off[F + 1];
  const uint64_t stream_off[S + 1] = {0, 30, 60};
  size_t n = 0;
  off[0] = 0;
  for (int f = 0; f < F; ++f) {
    const int clock_cells = f < 30 ? 3 : 2, object_cells = (f >= 10 && f < 20) ? 4 : 0;
    for (int c = 0; c < clock_cells + object_cells; ++c)
      for (int k = 0; k < 2; ++k) {                /* two votes per cell (VECTORS_NEEDED 2) */
        mt_mv *v = &mv[n++];
        const int gx = c < clock_cells ? 100 + c : 40 + (c - clock_cells), gy = c < clock_cells ? 0 : 30;
        v->dst_x = (int16_t)(16 * gx + 8);
        v->dst_y = (int16_t)(16 * gy + 8);
        v->src_x = (int16_t)(v->dst_x - 6);
        v->src_y = v->dst_y;
        v->w = v->h = 8;
        v->source = -1;
      }
    off[f + 1] = n;
  }
  uint8_t has_sd[F];
  memset(has_sd, 1, sizeof has_sd);
  const size_t plane = (size_t)S * p.grid_h * p.grid_w;
  uint32_t *active = malloc(plane * sizeof *active), *centre = malloc(plane * sizeof *centre), frames[S];
#define AT(map, s, x, y) map[((size_t)(s) * p.grid_h + (y)) * p.grid_w + (x)]

  CHECK(mtgpu_activity_map(ctx, mv, off, has_sd, F, stream_off, S, 0, active, centre, frames));
  printf("all frames:  stream 0: %u frames, clock cell (101, 0) centre in %u, object cell (41, 30) centre in %u\n", frames[0],
         AT(centre, 0, 101, 0), AT(centre, 0, 41, 30));
  int ok = frames[0] == 30 && frames[1] == 30 && AT(centre, 0, 101, 0) == 30 && AT(centre, 0, 41, 30) == 10 &&
           AT(active, 1, 100, 0) == 30 && AT(active, 1, 102, 0) == 0 && AT(centre, 1, 41, 30) == 0;
  uint64_t row0 = 0, all = 0;
  for (int y = 0; y < p.grid_h; ++y)
    for (int x = 0; x < p.grid_w; ++x) {
      all += AT(centre, 0, x, y);
      if (y == 0) row0 += AT(centre, 0, x, y);
    }
  printf("stream 0: %.0f %% of the centre counts lie in row 0 — the rows a VERTICAL_MASK would drop\n", 100.0 * row0 / all);

  /* only the frames the trimmer keeps: centre count >= max(1, CLUSTERS_NEEDED) */
  const uint32_t keep = p.clusters_needed < 1 ? 1u : (uint32_t)p.clusters_needed;
  CHECK(mtgpu_activity_map(ctx, mv, off, has_sd, F, stream_off, S, keep, NULL, centre, frames));
  printf("kept frames: stream 0: %u, stream 1: %u\n", frames[0], frames[1]);
  ok = ok && frames[0] == 30 && frames[1] == 30 && AT(centre, 1, 100, 0) == 30;

  mtgpu_destroy(ctx);
  free(mv); free(active); free(centre);
  return ok ? 0 : 3;
}
