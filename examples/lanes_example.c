/* lanes_example.c — a direction plane: a camera over a two-way road on a 12 x 8 grid.  The upper half of the picture is
 * the far lane, where traffic goes west; the lower half is the near lane, where anything goes.  A car drives EAST in the
 * upper half through frames 10 .. 19 — the wrong way for its lane — and another drives east in the lower half through
 * frames 40 .. 49, which is ordinary there.  One allow byte for the whole picture (mtgpu_dir.h) cannot tell the two
 * apart; a plane of one byte per cell can.  Here the plane lets everything but E, NE and SE vote in the upper rows and
 * everything in the lower rows: it keeps the ordinary car and drops the other.  (Inverted, it is the wrong-way detector.)
 *
 *   gcc -std=c11 -Iinclude examples/lanes_example.c -o lanes_example \
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

static void add_cell(mt_mv *mv, size_t *n, int gx, int gy, int dx, int dy) {
  for (int k = 0; k < 2; ++k) {                  /* two votes per cell (VECTORS_NEEDED 2) */
    mt_mv *v = &mv[(*n)++];
    v->dst_x = (int16_t)(16 * gx + 8);
    v->dst_y = (int16_t)(16 * gy + 8);
    v->src_x = (int16_t)(v->dst_x - dx);
    v->src_y = (int16_t)(v->dst_y - dy);
    v->w = v->h = 8;
    v->source = -1;
  }
}

/* the frames one plane keeps, and the segments the merge makes of them */
static int run(mtgpu_ctx *ctx, const mt_mv *mv, const uint64_t *off, const uint8_t *has_sd, const uint8_t *plane, const char *label,
               int *kept, uint64_t *segments) {
  uint8_t flags[F];
  uint32_t centres[F];
  CHECK(mtgpu_scan_frames_lanes(ctx, mv, off, has_sd, F, NULL, 0, plane, flags, centres, NULL));
  double ts[F];
  uint64_t n = 0;
  for (int f = 0; f < F; ++f)
    if (flags[f]) ts[n++] = f / 25.0;
  const mt_merge_params mp = {0.2, 0.04, F / 25.0, 5.0};
  mt_segment seg[8];
  mt_merge_result res;
  CHECK(mtgpu_merge_segments(ctx, ts, n, &mp, 0, seg, 8, &res));
  *kept = (int)n;
  *segments = res.n_segments;
  printf("%-28s %2d frames kept, %llu segment(s)", label, *kept, (unsigned long long)res.n_segments);
  for (uint64_t s = 0; s < res.n_segments && s < 8; ++s) printf("  [%.2f, %.2f]", seg[s].start, seg[s].end);
  printf("\n");
  return 0;
}

int main(void) {
  /* 192 x 128 pixels in 16-pixel blocks: 12 x 8 cells; reference code defaults but no vertical mask */
  mt_scan_params p;
  CHECK(mtgpu_params_from_config(&p, 16 * GW, 16 * GH, 16.0, 16, 4, 2, 2, 0.0f));
  mtgpu_lanes_plan plan;
  CHECK(mtgpu_lanes_preview(&p, 163840, &plan));
  if (p.grid_w != GW || p.grid_h != GH || plan.plane_bytes != GW * GH) {
    fprintf(stderr, "unexpected grid %d x %d, %d bytes per plane\n", p.grid_w, p.grid_h, plan.plane_bytes);
    return 1;
  }
  mtgpu_ctx *ctx = NULL;
  CHECK(mtgpu_create(&p, 0, &ctx));

  /* both cars: three cells in a row, two votes each, moving east by 6 pixels; the first in row 2, the second in row 5 */
  mt_mv *mv = calloc((size_t)F * 6, sizeof *mv);
  uint64_t off[F + 1];
  uint8_t has_sd[F];
  size_t n = 0;
  off[0] = 0;
  for (int f = 0; f < F; ++f) {
    if (f >= 10 && f < 20)
      for (int c = 0; c < 3; ++c) add_cell(mv, &n, 2 + (f - 10) / 2 + c, 2, 6, 0);
    if (f >= 40 && f < 50)
      for (int c = 0; c < 3; ++c) add_cell(mv, &n, 2 + (f - 40) / 2 + c, 5, 6, 0);
    off[f + 1] = n;
    has_sd[f] = 1;
  }

  /* sectors clockwise from E: E 0, SE 1, S 2, SW 3, W 4, NW 5, N 6, NE 7.  plane[y * GW + x]: the byte of cell (x, y) */
  uint8_t everything[GW * GH], plane[GW * GH];
  memset(everything, MTGPU_DIR_ALL, sizeof everything);
  for (int y = 0; y < GH; ++y)
    for (int x = 0; x < GW; ++x) plane[y * GW + x] = y < GH / 2 ? (uint8_t)(MTGPU_DIR_ALL & ~(1 << 0 | 1 << 7 | 1 << 1)) : MTGPU_DIR_ALL;

  int kept_all, kept_plane;
  uint64_t seg_all, seg_plane;
  printf("plane scan: %d lanes, LDS %d bytes, %s, %d bytes per plane\n", plan.workgroup, plan.lds_bytes,
         plan.staged ? "the plane's rows staged in LDS" : "the plane read from memory", plan.plane_bytes);
  if (run(ctx, mv, off, has_sd, everything, "0xFF everywhere", &kept_all, &seg_all)) return 1;
  if (run(ctx, mv, off, has_sd, plane, "upper half: not E, NE, SE", &kept_plane, &seg_plane)) return 1;
  const int ok = kept_all == 20 && seg_all == 2 && kept_plane == 10 && seg_plane == 1;

  free(mv);
  mtgpu_destroy(ctx);
  if (!ok) {
    fprintf(stderr, "unexpected counts\n");
    return 1;
  }
  return 0;
}
