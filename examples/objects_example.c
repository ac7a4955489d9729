/* objects_example.c — object lists: a truck of eight cells stands at a gate in all 60 frames, rain leaves one pair of
 * active cells in every frame, and a person of three cells walks in during frames 20 .. 39.  The largest blob
 * (mtgpu_blobs.h) is the truck throughout: it cannot see the person.  The object scan lists both — a size and a box each,
 * the larger first — and "at least 2 things of at least 3 cells" (src/motion_scanner.cpp:288 with one more term) keeps
 * exactly the twenty frames with the person.
 *
 *   gcc -std=c11 -Iinclude examples/objects_example.c -o objects_example \
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
  /* 1080p (a grid of 120 x 68 cells), reference code defaults with CLUSTERS_NEEDED 1 */
  enum { F = 60, K = 4, GW = 120 };
  mt_scan_params p;
  CHECK(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 2, 1, 0.05f));
  mtgpu_objects_plan plan;
  CHECK(mtgpu_objects_preview(&p, K, 163840, &plan));
  mtgpu_ctx *ctx = NULL;
  CHECK(mtgpu_create(&p, 0, &ctx));

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
    for (int c = 0; c < 8; ++c) add_cell(mv, &n, 40 + (c & 3), 30 + (c >> 2));      /* the truck: 4 x 2 cells at (40, 30) */
    add_cell(mv, &n, 20, 10);                                                       /* rain: one pair */
    add_cell(mv, &n, 21, 10);
    if (f >= 20 && f < 40)
      for (int c = 0; c < 3; ++c) add_cell(mv, &n, 60 + f, 20 + c);                 /* the person: 1 x 3 cells, walking right */
    off[f + 1] = n;
    has_sd[f] = 1;
  }

  uint8_t flags[F];
  uint32_t centres[F], blobs[F], objects[F];
  static mt_object list[F * K];
  /* no keep mask: stream_off NULL, n_streams 0, keep NULL.  An object has at least 3 cells; a frame needs 2 of them. */
  CHECK(mtgpu_scan_frames_objects(ctx, mv, off, has_sd, F, NULL, 0, NULL, K, 3, 2, flags, centres, blobs, objects, list));

  int kept = 0;
  for (int f = 0; f < F; ++f) kept += flags[f];
  printf("LDS %d bytes, %d lanes\n", plan.lds_bytes, plan.workgroup);
  for (int f = 5; f <= 25; f += 20) {
    printf("frame %d: %u centres in %u blobs, %u objects:", f, centres[f], blobs[f], objects[f]);
    for (int j = 0; j < K && list[f * K + j].cells; ++j) {
      const mt_object *o = &list[f * K + j];
      printf(" %u cells at (%u, %u) .. (%u, %u)%s", o->cells, (unsigned)o->x0, (unsigned)o->y0, (unsigned)o->x1, (unsigned)o->y1,
             j + 1 < K && o[1].cells ? "," : "");
    }
    printf("\n");
  }
  printf("motion frames: %d of %d with MIN_OBJECTS 2 at MIN_BLOB_CELLS 3\n", kept, F);
  const mt_object *a = &list[25 * K], *b = a + 1, *c = a + 2, *d = a + 3;
  const int ok = centres[5] == 10 && blobs[5] == 2 && objects[5] == 1 && list[5 * K + 2].cells == 0 && list[5 * K + 2].first == 0xFFFFFFFFu &&
                 centres[25] == 13 && blobs[25] == 3 && objects[25] == 2 && a->cells == 8 && a->first == 30u * GW + 40u && a->x0 == 40 &&
                 a->y0 == 30 && a->x1 == 43 && a->y1 == 31 && b->cells == 3 && b->first == 20u * GW + 85u && b->x0 == 85 && b->y0 == 20 &&
                 b->x1 == 85 && b->y1 == 22 && c->cells == 2 && c->x0 == 20 && c->x1 == 21 && d->cells == 0 && d->x0 == 0xFFFF && kept == 20 &&
                 flags[19] == 0 && flags[20] == 1 && flags[39] == 1 && flags[40] == 0;

  free(mv);
  mtgpu_destroy(ctx);
  if (!ok) {
    fprintf(stderr, "unexpected counts\n");
    return 1;
  }
  return 0;
}
