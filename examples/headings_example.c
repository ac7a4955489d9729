/* headings_example.c — object headings: a one-way street.  A car of twelve cells drives E in all 60 frames; a walker of
 * four cells goes W, against the traffic, during frames 20 .. 39.  The direction scan's rose (mtgpu_dir.h) of such a
 * frame has two lobes and no box; the object scan (mtgpu_objects.h) has two boxes and no direction.  The heading scan
 * gives every listed object its own rose, record count and summed displacement, and with every heading but E allowed,
 * "at least 1 object of at least 3 cells" keeps exactly the twenty frames with the walker.
 *
 *   gcc -std=c11 -Iinclude examples/headings_example.c -o headings_example \
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

static void add_cell(mt_mv *mv, size_t *n, int gx, int gy, int votes, int dx) {
  for (int k = 0; k < votes; ++k) {
    mt_mv *v = &mv[(*n)++];
    v->dst_x = (int16_t)(16 * gx + 8);
    v->dst_y = (int16_t)(16 * gy + 8);
    v->src_x = (int16_t)(v->dst_x - dx);
    v->src_y = v->dst_y;
    v->w = v->h = 8;
    v->source = -1;
  }
}

int main(void) {
  /* 1080p (a grid of 120 x 68 cells), MV_THRESHOLD_SQ 4, VECTORS_NEEDED 2, CLUSTERS_NEEDED 1 */
  enum { F = 60, K = 4 };
  static const char *const names[8] = {"E", "SE", "S", "SW", "W", "NW", "N", "NE"};
  mt_scan_params p;
  CHECK(mtgpu_params_from_config(&p, 1920, 1080, 4.0, 16, 4, 2, 1, 0.05f));
  mtgpu_headings_plan plan;
  CHECK(mtgpu_headings_preview(&p, K, 163840, &plan));
  mtgpu_ctx *ctx = NULL;
  CHECK(mtgpu_create(&p, 0, &ctx));

  mt_mv *mv = calloc((size_t)F * 48, sizeof *mv);
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
    for (int c = 0; c < 12; ++c) add_cell(mv, &n, 30 + f + c % 6, 30 + c / 6, 3, 8);     /* the car: 6 x 2 cells, 8 pixels E per frame */
    if (f >= 20 && f < 40)
      for (int c = 0; c < 4; ++c) add_cell(mv, &n, 100 - f + (c & 1), 40 + (c >> 1), 2, -3);   /* the walker: 2 x 2 cells, 3 pixels W */
    off[f + 1] = n;
    has_sd[f] = 1;
  }

  uint8_t flags[F];
  uint32_t centres[F], objects[F], allowed[F];
  static mt_object list[F * K];
  static mt_heading motion[F * K];
  /* no keep mask: stream_off NULL, n_streams 0, keep NULL.  An object has at least 3 cells; every heading but E is
   * allowed; a frame needs one allowed object. */
  const int allow = 0xFF & ~(1 << 0);
  CHECK(mtgpu_scan_frames_headings(ctx, mv, off, has_sd, F, NULL, 0, NULL, K, 3, 1, allow, flags, centres, NULL, objects, list, motion,
                                   allowed));

  int kept = 0;
  for (int f = 0; f < F; ++f) kept += flags[f];
  printf("LDS %d bytes, %d lanes\n", plan.lds_bytes, plan.workgroup);
  printf("frame 25: %u centres, %u objects, %u allowed\n", centres[25], objects[25], allowed[25]);
  for (int j = 0; j < K && list[25 * K + j].cells; ++j) {
    const mt_object *o = &list[25 * K + j];
    const mt_heading *h = &motion[25 * K + j];
    printf("object %d: %u cells, heading %s, %u records, mean (%+.2f, %+.2f)\n", j, o->cells,
           h->heading == MT_HEADING_NONE ? "none" : names[h->heading & 7u], h->records, (double)h->sum_dx / (double)h->records,
           (double)h->sum_dy / (double)h->records);
  }
  printf("against the traffic: %d of %d frames\n", kept, F);
  const mt_heading *a = &motion[25 * K], *b = a + 1, *c = a + 2;
  const int ok = centres[25] == 16 && objects[25] == 2 && allowed[25] == 1 && allowed[5] == 0 && a->heading == 0 && a->n[0] == 36 &&
                 a->records == 36 && a->sum_dx == 288 && a->sum_dy == 0 && b->heading == 4 && b->n[4] == 8 && b->records == 8 &&
                 b->sum_dx == -24 && b->sum_dy == 0 && c->heading == MT_HEADING_NONE && c->records == 0 && c->reserved == 0 &&
                 motion[5 * K + 1].heading == MT_HEADING_NONE && kept == 20 && flags[19] == 0 && flags[20] == 1 && flags[39] == 1 &&
                 flags[40] == 0;

  free(mv);
  mtgpu_destroy(ctx);
  if (!ok) {
    fprintf(stderr, "unexpected counts\n");
    return 1;
  }
  return 0;
}
