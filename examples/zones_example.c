/* zones_example.c — ignore zones: a burnt-in clock in the top right corner moves in every frame and keeps the whole
 * recording "in motion".  VERTICAL_MASK (src/motion_scanner.cpp:237-238, 262) could only cut the full-width strip the
 * clock sits in; a keep mask ignores its four cells alone.  One masked scan returns every frame's centre count with
 * and without the zone from one read of the records.
 *
 *   gcc -std=c11 -Iinclude examples/zones_example.c -o zones_example \
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
  /* 1080p, reference code defaults but no vertical mask: the clock's row 4 would be analysed either way */
  mt_scan_params p;
  CHECK(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 2, 2, 0.0f));
  mtgpu_zones_plan plan;
  CHECK(mtgpu_zones_preview(&p, 163840, &plan));
  mtgpu_ctx *ctx = NULL;
  CHECK(mtgpu_create(&p, 0, &ctx));

  /* 60 frames: the clock (cells 110 .. 113 of row 4) in every frame, an object (cells 40 .. 42 of row 30) in 10 .. 19 */
  enum { F = 60 };
  mt_mv *mv = calloc((size_t)F * 14, sizeof *mv);
  uint64_t off[F + 1];
  uint8_t has_sd[F];
  size_t n = 0;
  off[0] = 0;
  for (int f = 0; f < F; ++f) {
    for (int c = 0; c < 4; ++c) add_cell(mv, &n, 110 + c, 4);
    if (f >= 10 && f < 20)
      for (int c = 0; c < 3; ++c) add_cell(mv, &n, 40 + c, 30);
    off[f + 1] = n;
    has_sd[f] = 1;
  }

  /* one stream, one keep plane of grid_h x W words: everything kept but the clock's cells */
  const uint64_t stream_off[2] = {0, F};
  uint64_t *keep = malloc(sizeof(uint64_t) * (size_t)plan.keep_words_per_stream);
  memset(keep, 0xff, sizeof(uint64_t) * (size_t)plan.keep_words_per_stream);
  for (int x = 110; x < 114; ++x) keep[4 * plan.keep_words_per_row + (x >> 6)] &= ~(1ull << (x & 63));

  uint8_t flags[F];
  uint32_t centres[F], centres_all[F];
  CHECK(mtgpu_scan_frames_zones(ctx, mv, off, has_sd, F, stream_off, 1, keep, flags, centres, centres_all));

  int kept = 0, kept_all = 0;
  for (int f = 0; f < F; ++f) {
    kept += flags[f];
    kept_all += centres_all[f] >= 2;
  }
  printf("keep mask: %d words per row, %d per stream; LDS %d bytes\n", plan.keep_words_per_row, plan.keep_words_per_stream,
         plan.lds_bytes);
  printf("frame 5:  %u centres without the zone, %u with\n", centres_all[5], centres[5]);
  printf("frame 15: %u centres without the zone, %u with\n", centres_all[15], centres[15]);
  printf("motion frames: %d of %d without the zone, %d with\n", kept_all, F, kept);
  const int ok = centres_all[5] == 4 && centres[5] == 0 && centres_all[15] == 7 && centres[15] == 3 && kept_all == F && kept == 10;

  free(keep);
  free(mv);
  mtgpu_destroy(ctx);
  if (!ok) {
    fprintf(stderr, "unexpected counts\n");
    return 1;
  }
  return 0;
}
