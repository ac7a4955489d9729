/*
 * pipe_dir_example.c — the direction filter on the decode path, plain C (include/mtgpu_pipe_dir.h).
 *
 * The one-way street of dir_example.c, fed frame by frame through a pipe: a car drives east through frames 10 .. 19, in
 * frames 40 .. 49 somebody walks west, against the traffic.  This camera also burns a clock into the top left corner,
 * and the encoder gives its flickering digits small vectors pointing down in every frame.  With every sector allowed the
 * pipe keeps every frame.  Ignoring W, NW and SW does not help: the clock still votes.  Ignoring E, NE, SE and S under a
 * keep mask that clears the clock keeps the walker alone — the byte handles the traffic, the mask the overlay.
 *
 *   cc -std=c11 -Iinclude examples/pipe_dir_example.c -L<package dir> -lmtgpu -Wl,-rpath,<package dir> -o pipe_dir_example
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

enum { F = 60 };

static size_t g_kept = 0;
static uint32_t g_words[F];
static int g_inflight = 0;

/* wait for the oldest batch, count its motion frames (:382-383), keep every frame's count word, free the batch */
static int collect(mtgpu_pipe *pipe) {
  mtgpu_batch *b = NULL;
  const uint8_t *flags = NULL;
  const uint64_t *tags = NULL;
  const uint32_t *words = NULL;
  uint32_t n = 0;
  CHECK(mtgpu_pipe_collect(pipe, &b, &flags, NULL, &tags, &n));
  CHECK(mtgpu_batch_centres(b, &words));
  for (uint32_t i = 0; i < n; ++i) {
    if (flags[i]) ++g_kept;
    g_words[tags[i]] = words[i];
  }
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

/* the decode loop */
static int scan(mtgpu_pipe *pipe) {
  static mt_mv side_data[64];                    /* stands for the AVFrame's side data */
  mtgpu_batch *cur = NULL;
  g_kept = 0;
  for (int f = 0; f < F; ++f) {
    size_t n = 0;
    memset(side_data, 0, sizeof side_data);
    for (int c = 0; c < 4; ++c) add_cell(side_data, &n, 5 + c, 3, 0, 5);                  /* the clock */
    if (f >= 10 && f < 20)
      for (int c = 0; c < 3; ++c) add_cell(side_data, &n, 30 + (f - 10) + c, 30, 6, 0);   /* the car */
    if (f >= 40 && f < 50)
      for (int c = 0; c < 2; ++c) add_cell(side_data, &n, 80 - (f - 40) + c, 34, -5, 1);  /* the walker */
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
  return 0;
}

int main(void) {
  /* 1080p, reference code defaults but no vertical mask */
  mt_scan_params p;
  CHECK(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 2, 2, 0.0f));
  mtgpu_ctx *ctx = NULL;
  CHECK(mtgpu_create(&p, 0, &ctx));
  mtgpu_pipe *pipe = NULL;
  CHECK(mtgpu_pipe_create_layout(ctx, 1024, 16, 3, MT_LAYOUT_COMPACT8 | MT_LAYOUT_ZERO_COPY | MT_LAYOUT_CENTRES, &pipe));

  /* the keep plane: 68 rows of two 64-bit words, every cell kept but the clock's */
  static uint64_t keep[68 * 2];
  for (int i = 0; i < 68 * 2; ++i) keep[i] = ~0ull;
  for (int x = 5; x < 9; ++x) keep[3 * 2 + (x >> 6)] &= ~(1ull << (x & 63));

  /* sectors clockwise from E: E 0, SE 1, S 2, SW 3, W 4, NW 5, N 6, NE 7 */
  size_t kept[3];
  if (mtgpu_pipe_dir(pipe, NULL, NULL) != 0) return 2;
  CHECK(mtgpu_pipe_set_dir(pipe, 1, MTGPU_DIR_ALL, MT_PIPE_REPORT_CENTRES));
  if (scan(pipe)) return 1;
  kept[0] = g_kept;
  printf("all sectors:                      motion frames %zu\n", g_kept);

  CHECK(mtgpu_pipe_set_dir(pipe, 1, MTGPU_DIR_ALL & ~(1 << 4 | 1 << 5 | 1 << 3), MT_PIPE_REPORT_CENTRES));
  int32_t allow = -1;
  int report = -1;
  if (mtgpu_pipe_dir(pipe, &allow, &report) != 1 || allow != 0xC7 || report != MT_PIPE_REPORT_CENTRES) return 2;
  if (scan(pipe)) return 1;
  kept[1] = g_kept;
  printf("--ignore W,NW,SW:                 motion frames %zu  (the clock still votes)\n", g_kept);

  CHECK(mtgpu_pipe_set_keep(pipe, keep));
  CHECK(mtgpu_pipe_set_dir(pipe, 1, MTGPU_DIR_ALL & ~(1 << 0 | 1 << 7 | 1 << 1 | 1 << 2), MT_PIPE_REPORT_SECTORS));
  if (scan(pipe)) return 1;
  kept[2] = g_kept;
  printf("--ignore E,NE,SE,S, clock masked: motion frames %zu\n", g_kept);
  /* the sector word: the present byte, the dominant sector, its count — under the mask, whatever the byte says */
  const uint32_t car = g_words[15], walker = g_words[45], quiet = g_words[30];
  printf("  frame 15: present 0x%02x dominant %u count %u; frame 45: present 0x%02x dominant %u count %u; frame 30: %u\n", car & 0xff,
         (car >> 8) & 7, car >> 11, walker & 0xff, (walker >> 8) & 7, walker >> 11, quiet);

  CHECK(mtgpu_pipe_set_dir(pipe, 0, 0, 0));       /* the next recording: the masked scan alone, as before */
  if (mtgpu_pipe_dir(pipe, NULL, NULL) != 0 || mtgpu_pipe_has_keep(pipe) != 1) return 2;
  mtgpu_pipe_destroy(pipe);
  mtgpu_destroy(ctx);
  const int ok = kept[0] == 60 && kept[1] == 60 && kept[2] == 10 && car == (0x01u | 0u << 8 | 6u << 11) &&
                 walker == (0x10u | 4u << 8 | 4u << 11) && quiet == 0;
  if (!ok) {
    fprintf(stderr, "unexpected counts\n");
    return 3;
  }
  return 0;
}
