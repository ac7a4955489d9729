/* blobs_example.c — motion blobs: rain leaves four unrelated pairs of active cells in every frame — eight "clusters",
 * as many as the reference's per-cell count (src/motion_scanner.cpp:272-294) sees when one object of eight cells walks
 * through frames 10 .. 19.  CLUSTERS_NEEDED = 8 keeps all 60 frames; a minimum object size of 8 cells keeps the ten with
 * the object, and the box says where it is.
 *
 *   gcc -std=c11 -Iinclude examples/blobs_example.c -o blobs_example \
 *       -Lmotion-estimated-video-trimmer_amd -lmtgpu -Wl,-rpath,$PWD/motion-estimated-video-trimmer_amd
 */
#include <stdio.h>
#include <stdlib.h>

#include "mtgpu.h"

#define CHECK(call)                                                        \
  do {                                                                     \
    int rc_ = (call);                                                      \
    if (rc_ != MT_OK) {                                                    \
      fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mtgpu_last_error());   \
      return 1;                                                            \
    }                                                                      \
  } while (0)

static void add_cell(mt_mv *mv, size_t *n, int gx, int gy) {
  for (int k = 0; k < 2; ++k) {                  /* two votes per cell (VECTORS_NEEDED 2) */
    mt_mv *v = &mv[(*n)++];
    v->dst_x = (int16_t)(16 * gx + 8);
    v->dst_y = (int16_t)(16 * gy + 8);
    v->src_x = (int16_t)(v->dst_x - 6);
    v->src_y = v->dst_y;
    v->w = v->h = 8;
    v->source = -1;
  }
}

int main(void) {
  /* 1080p, reference code defaults with CLUSTERS_NEEDED 8 */
  mt_scan_params p;
  CHECK(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 2, 8, 0.05f));
  mtgpu_blobs_plan plan;
  CHECK(mtgpu_blobs_preview(&p, 163840, &plan));
  mtgpu_ctx *ctx = NULL;
  CHECK(mtgpu_create(&p, 0, &ctx));

  /* 60 frames: four pairs of rain in every frame, an object of 4 x 2 cells at (40 + f, 30) in frames 10 .. 19 */
  enum { F = 60 };
  static const int rain[4][2] = {{20, 10}, {50, 12}, {80, 14}, {100, 40}};
  mt_mv *mv = calloc((size_t)F * 32, sizeof *mv);
  if (!mv) {
    fprintf(stderr, "out of memory\n");
    mtgpu_destroy(ctx);
    return 1;
  }
  uint64_t off[F + 1];
  uint8_t has_sd[F];
  size_t n = 0;
  off[0] = 0;
  for (int f = 0; f < F; ++f) {
    for (int r = 0; r < 4; ++r) {
      add_cell(mv, &n, rain[r][0], rain[r][1]);
      add_cell(mv, &n, rain[r][0] + 1, rain[r][1]);
    }
    if (f >= 10 && f < 20)
      for (int c = 0; c < 8; ++c) add_cell(mv, &n, 40 + f + (c & 3), 30 + (c >> 2));
    off[f + 1] = n;
    has_sd[f] = 1;
  }

  uint8_t flags[F];
  uint32_t centres[F], blobs[F], largest[F];
  mt_blob_box box[F];
  /* no keep mask: stream_off NULL, n_streams 0, keep NULL */
  CHECK(mtgpu_scan_frames_blobs(ctx, mv, off, has_sd, F, NULL, 0, NULL, 8, flags, centres, blobs, largest, box));

  int by_cells = 0, by_blob = 0;
  for (int f = 0; f < F; ++f) {
    by_cells += centres[f] >= 8;
    by_blob += flags[f];
  }
  printf("LDS %d bytes, %d lanes\n", plan.lds_bytes, plan.workgroup);
  printf("frame 5:  %u centres in %u blobs, largest %u\n", centres[5], blobs[5], largest[5]);
  printf("frame 15: %u centres in %u blobs, largest %u at (%u, %u) .. (%u, %u)\n", centres[15], blobs[15], largest[15],
         (unsigned)box[15].x0, (unsigned)box[15].y0, (unsigned)box[15].x1, (unsigned)box[15].y1);
  printf("motion frames: %d of %d with CLUSTERS_NEEDED 8, %d with MIN_BLOB_CELLS 8\n", by_cells, F, by_blob);
  const int ok = centres[5] == 8 && blobs[5] == 4 && largest[5] == 2 && centres[15] == 16 && blobs[15] == 5 && largest[15] == 8 &&
                 box[15].x0 == 55 && box[15].y0 == 30 && box[15].x1 == 58 && box[15].y1 == 31 && by_cells == F && by_blob == 10;

  free(mv);
  mtgpu_destroy(ctx);
  if (!ok) {
    fprintf(stderr, "unexpected counts\n");
    return 1;
  }
  return 0;
}
