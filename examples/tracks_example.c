/* tracks_example.c — object tracks: twelve frames with two movers and one flicker.  Mover A (six cells) walks right
 * through frames 0 .. 5; mover B (four cells) walks down through frames 2 .. 9 — as the second-largest blob while A is
 * in the picture, as the largest afterwards; frame 10 is quiet, and in frame 11 a two-cell blob flickers once.  The
 * lists are what an object scan (mtgpu_scan_frames_objects) returns for such a picture.  The call links each list to
 * the one before and tells how deep every track gets; MIN_TRACK = 7 keeps the frames in which B is seen and drops both
 * A's first two frames and the flicker.
 *
 *   gcc -std=c11 -Iinclude examples/tracks_example.c -o tracks_example \
 *       -Lmotion-estimated-video-trimmer_amd -lmtgpu -Wl,-rpath,$PWD/motion-estimated-video-trimmer_amd
 */
#include <stdio.h>

#include "mtgpu.h"

#define CHECK(call)                                                        \
  do {                                                                     \
    int rc_ = (call);                                                      \
    if (rc_ != MT_OK) {                                                    \
      fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mtgpu_last_error());   \
      return 1;                                                            \
    }                                                                      \
  } while (0)

enum { F = 12, K = 4 };

static mt_object blob(uint32_t cells, uint16_t x0, uint16_t y0, uint16_t x1, uint16_t y1) {
  mt_object o = {cells, (uint32_t)y0 * 120u + x0, x0, y0, x1, y1};
  return o;
}

int main(void) {
  mt_scan_params p;
  CHECK(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 2, 8, 0.05f));
  mtgpu_tracks_plan plan;
  CHECK(mtgpu_tracks_preview(K, &plan));
  mtgpu_ctx *ctx = NULL;
  CHECK(mtgpu_create(&p, 0, &ctx));

  uint8_t flags[F];
  mt_object list[F * K];
  const mt_object none = {0, 0xFFFFFFFFu, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF};
  for (int f = 0; f < F; ++f) {
    int n = 0;
    for (int j = 0; j < K; ++j) list[f * K + j] = none;
    if (f <= 5) list[f * K + n++] = blob(6, (uint16_t)(2 + f), 2, (uint16_t)(4 + f), 3);                 /* A */
    if (f >= 2 && f <= 9) list[f * K + n++] = blob(4, 20, (uint16_t)(4 + f), 21, (uint16_t)(5 + f));    /* B */
    if (f == 11) list[f * K + n++] = blob(2, 30, 15, 31, 15);                                            /* the flicker */
    flags[f] = n > 0;
  }
  const uint64_t stream_off[2] = {0, F};

  uint8_t pred[F * K];
  uint32_t age[F * K], id[F * K], len[F * K], track[F];
  /* an object is a blob of at least one cell; no dropout is bridged; linked boxes lie at most one cell apart */
  CHECK(mtgpu_track_objects(ctx, flags, NULL, list, K, F, stream_off, 1, 1, 0, 1, 1, pred, age, id, len, track, NULL));

  int tracks = 0;
  for (int e = 0; e < F * K; ++e)
    if (age[e] == 1) ++tracks;
  printf("%d lanes, %d frames per tile, %d workspace words per entry\n", plan.workgroup, plan.frames_per_tile, plan.work_words_per_entry);
  printf("%d tracks\n", tracks);
  for (int e = 0; e < F * K; ++e)
    if (age[e] == 1) printf("track %u: %u frames, from frame %d entry %d\n", id[e], len[e], e / K, e % K);
  for (int f = 0; f < F; ++f) {
    printf("frame %2d: longest track %u;", f, track[f]);
    for (int j = 0; j < K; ++j)
      if (age[f * K + j]) {
        printf("  [%d] track %u age %u", j, id[f * K + j], age[f * K + j]);
        if (pred[f * K + j] != MT_TRACK_NO_PRED) printf(" <- [%u]", pred[f * K + j]);
      }
    printf("\n");
  }

  static const uint32_t levels[4] = {1, 2, 7, 9};
  int kept[4];
  for (int i = 0; i < 4; ++i) {
    uint8_t out[F];
    CHECK(mtgpu_track_objects(ctx, flags, NULL, list, K, F, stream_off, 1, 1, 0, 1, levels[i], NULL, NULL, NULL, NULL, NULL, out));
    kept[i] = 0;
    for (int f = 0; f < F; ++f) kept[i] += out[f];
    printf("MIN_TRACK %u: %d motion frames\n", levels[i], kept[i]);
  }

  mtgpu_destroy(ctx);
  if (tracks != 3 || kept[0] != 11 || kept[1] != 10 || kept[2] != 8 || kept[3] != 0 || pred[6 * K] != 1 || id[6 * K] != 9) {
    fprintf(stderr, "unexpected counts\n");
    return 1;
  }
  return 0;
}
