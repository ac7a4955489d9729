/* gmc_blobs_example.c — the compensated blob scan: a camera pans by (9, 3) over rows 20 .. 39 of a 1080p picture.  Frame
 * 0 also holds four unrelated pairs of cells that move on their own (rain, foliage), frame 1 one object of 4 x 2 cells;
 * both move 5 pixels faster than the pan.  Three scans side by side:
 *   the blob scan             sees the panned region as ONE blob of 2360 cells in both frames;
 *   the compensated scan      sees 8 centres in both frames: CLUSTERS_NEEDED = 8 keeps both;
 *   the compensated blob scan sees 4 blobs of 2 cells in frame 0 and 1 blob of 8 in frame 1: MIN_BLOB_CELLS = 8 keeps
 *                             the object and drops the pairs.
 *
 *   gcc -std=c11 -Iinclude examples/gmc_blobs_example.c -o gmc_blobs_example \
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

/* 1: the cell belongs to frame f's objects */
static int is_object(int f, int x, int y) {
  if (f == 0) return (y == 25 || y == 30) && (x == 50 || x == 51 || x == 60 || x == 61);
  return (y == 25 || y == 26) && x >= 50 && x <= 53;
}

int main(void) {
  /* 1080p, reference code defaults with CLUSTERS_NEEDED 8 */
  mt_scan_params p;
  CHECK(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 2, 8, 0.05f));
  mtgpu_gmc_blobs_plan plan;
  CHECK(mtgpu_gmc_blobs_preview(&p, 163840, &plan));
  mtgpu_ctx *ctx = NULL;
  CHECK(mtgpu_create(&p, 0, &ctx));

  enum { F = 2 };
  mt_mv *mv = calloc((size_t)F * 120 * 20 * 2, sizeof *mv);
  if (!mv) {
    fprintf(stderr, "out of memory\n");
    mtgpu_destroy(ctx);
    return 1;
  }
  uint64_t off[F + 1];
  uint8_t has_sd[F] = {1, 1};
  size_t n = 0;
  off[0] = 0;
  for (int f = 0; f < F; ++f) {
    for (int y = 20; y < 40; ++y)
      for (int x = 0; x < 120; ++x) add_cell(mv, &n, x, y, is_object(f, x, y) ? 14 : 9, 3);
    off[f + 1] = n;
  }

  uint8_t fl_b[F], fl_g[F], fl_gb[F];
  uint32_t ce_b[F], bl_b[F], lg_b[F], ce_g[F], ce_gb[F], bl_gb[F], lg_gb[F];
  mt_blob_box box_b[F], box_gb[F];
  mt_gmc_info info[F];
  /* no keep mask: stream_off NULL, n_streams 0, keep NULL */
  CHECK(mtgpu_scan_frames_blobs(ctx, mv, off, has_sd, F, NULL, 0, NULL, 8, fl_b, ce_b, bl_b, lg_b, box_b));
  CHECK(mtgpu_scan_frames_gmc(ctx, mv, off, has_sd, F, MTGPU_GMC_DEFAULT_MAX_SHIFT, MTGPU_GMC_DEFAULT_MIN_SHARE_Q8, fl_g, ce_g, NULL));
  CHECK(mtgpu_scan_frames_gmc_blobs(ctx, mv, off, has_sd, F, NULL, 0, NULL, MTGPU_GMC_DEFAULT_MAX_SHIFT,
                                    MTGPU_GMC_DEFAULT_MIN_SHARE_Q8, 8, fl_gb, ce_gb, bl_gb, lg_gb, box_gb, info));

  printf("LDS %d bytes, %d lanes, %d bins per axis\n", plan.lds_bytes, plan.workgroup, plan.hist_bins);
  int ok = 1;
  for (int f = 0; f < F; ++f) {
    printf("frame %d  blobs: %u centres in %u blobs, largest %u, flag %d | gmc: %u centres, flag %d | gmc + blobs: vector (%d, %d), "
           "%u centres in %u blobs, largest %u at (%u, %u) .. (%u, %u), flag %d\n", f, ce_b[f], bl_b[f], lg_b[f], fl_b[f], ce_g[f],
           fl_g[f], info[f].gx, info[f].gy, ce_gb[f], bl_gb[f], lg_gb[f], (unsigned)box_gb[f].x0, (unsigned)box_gb[f].y0,
           (unsigned)box_gb[f].x1, (unsigned)box_gb[f].y1, fl_gb[f]);
    ok = ok && ce_b[f] == 2360 && bl_b[f] == 1 && lg_b[f] == 2360 && fl_b[f] == 1 && ce_g[f] == 8 && fl_g[f] == 1 && ce_gb[f] == 8 &&
         info[f].gx == 9 && info[f].gy == 3 && info[f].n_in == 4800 && info[f].n_x == 4784 && info[f].n_y == 4800;
  }
  ok = ok && bl_gb[0] == 4 && lg_gb[0] == 2 && fl_gb[0] == 0 && box_gb[0].x0 == 50 && box_gb[0].y0 == 25 && box_gb[0].x1 == 51 &&
       box_gb[0].y1 == 25 && bl_gb[1] == 1 && lg_gb[1] == 8 && fl_gb[1] == 1 && box_gb[1].x0 == 50 && box_gb[1].y0 == 25 &&
       box_gb[1].x1 == 53 && box_gb[1].y1 == 26;
  printf("motion frames with a minimum of 8: blobs %d, gmc %d, gmc + blobs %d of %d\n", fl_b[0] + fl_b[1], fl_g[0] + fl_g[1],
         fl_gb[0] + fl_gb[1], F);

  free(mv);
  mtgpu_destroy(ctx);
  if (!ok) {
    fprintf(stderr, "unexpected counts\n");
    return 1;
  }
  return 0;
}
