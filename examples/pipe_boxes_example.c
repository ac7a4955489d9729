/* pipe_boxes_example.c — persistence on the decode path: a pipe with MT_LAYOUT_BOXES (include/mtgpu_pipe_boxes.h) runs
 * the blob scan and reports, next to every flag, the largest blob's box; the flags and boxes of all batches are
 * concatenated and ONE mtgpu_persist_flags call per recording (include/mtgpu_persist.h) decides which motion frames
 * belong to a run of at least MIN_RUN — no state is carried from one batch to the next.
 *
 * The recording: 300 frames at 30 fps, a key frame every 30.  Frames 60 .. 149: "rain" — one blob of 4 x 2 cells that
 * passes the blob rule in every frame, but somewhere else each time.  Frames 200 .. 259: one object of 4 x 2 cells that
 * moves one cell a frame.  Without the boxes the rain is one long run and is kept; with them (reach 2) every rain frame
 * is a run of its own and MIN_RUN 3 leaves the object alone.  Plain C against include/mtgpu.h.
 *
 *   gcc -std=c11 -Iinclude examples/pipe_boxes_example.c -o pipe_boxes_example \
 *       -Lmotion-estimated-video-trimmer_amd -lmtgpu -Wl,-rpath,$PWD/motion-estimated-video-trimmer_amd
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

enum { F = 300, PER = 8, MIN_BLOB_CELLS = 3, MIN_RUN = 3, REACH = 2 };

/* the recording's results, concatenated over the batches in submission order */
static uint8_t g_flags[F], g_has_sd[F];
static mt_blob_box g_box[F];
static double g_pts[F];
static size_t g_n = 0;
static int g_inflight = 0;

/* wait for the oldest batch and append its flags, its boxes and (from the tags) which frames had side data */
static int collect(mtgpu_pipe *pipe) {
  mtgpu_batch *b = NULL;
  const uint8_t *flags = NULL;
  const double *pts = NULL;
  const uint64_t *tags = NULL;
  const struct mt_blob_box *box = NULL;
  uint32_t n = 0;
  CHECK(mtgpu_pipe_collect(pipe, &b, &flags, &pts, &tags, &n));
  CHECK(mtgpu_batch_boxes(b, &box));
  for (uint32_t i = 0; i < n; ++i, ++g_n) {
    g_flags[g_n] = flags[i];
    g_pts[g_n] = pts[i];
    g_has_sd[g_n] = (uint8_t)tags[i];
    /* a box is specified where the flag is set; everywhere else: the "no blob" box */
    if (flags[i]) g_box[g_n] = box[i];
    else memset(&g_box[g_n], 0xff, sizeof g_box[g_n]);
  }
  --g_inflight;
  CHECK(mtgpu_pipe_release(pipe, b));
  return 0;
}

static int scan(mtgpu_pipe *pipe) {
  mtgpu_batch *cur = NULL;
  for (int f = 0; f < F; ++f) {
    mt_mv side_data[PER];                          /* stands for the AVFrame's side data: dies with the frame */
    size_t n = 0;
    const int rain = f >= 60 && f < 150, object = f >= 200 && f < 260;
    memset(side_data, 0, sizeof side_data);
    if (rain || object) {
      const int gx0 = rain ? 10 + 35 * (f % 3) : 20 + (f - 200), gy0 = rain ? 10 + 20 * (f % 3) : 30;
      for (int k = 0; k < PER; ++k) {
        mt_mv *v = &side_data[n++];
        v->dst_x = (int16_t)(16 * (gx0 + k % 4) + 8);
        v->dst_y = (int16_t)(16 * (gy0 + k / 4) + 8);
        v->src_x = (int16_t)(v->dst_x - 6);
        v->src_y = v->dst_y;
      }
    }
    const int has_sd = (f % 30) != 0;              /* key frames export no MV side data */
    for (;;) {
      if (!cur) {
        int rc = mtgpu_pipe_acquire(pipe, &cur);
        if (rc == MT_ERR_BUSY) { if (collect(pipe)) return 1; continue; }   /* back-pressure */
        CHECK(rc);
      }
      /* the tag carries has_sd to the collecting side: persistence must know the key frames */
      int rc = mtgpu_batch_add_frame(cur, has_sd ? side_data : NULL, n * sizeof(mt_mv), has_sd, f / 30.0, (uint64_t)has_sd);
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
  mt_scan_params p;
  CHECK(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 1, 8, 0.05f));   /* VECTORS_NEEDED 1, CLUSTERS_NEEDED 8 */
  mtgpu_ctx *ctx = NULL;
  CHECK(mtgpu_create(&p, 0, &ctx));
  mtgpu_pipe *pipe = NULL;
  CHECK(mtgpu_pipe_create_layout(ctx, 4096, 16, 3, MT_LAYOUT_COMPACT8 | MT_LAYOUT_ZERO_COPY | MT_LAYOUT_BOXES, &pipe));
  CHECK(mtgpu_pipe_set_blobs(pipe, MIN_BLOB_CELLS, MT_PIPE_REPORT_CENTRES));
  if (scan(pipe)) return 1;
  mtgpu_pipe_destroy(pipe);
  if (g_n != F) return 2;

  const uint64_t stream_off[2] = {0, F};
  const mt_merge_params mp = {1.0, 0.5, F / 30.0, 5.0};   /* MAX_GAP_SEC, PADDING_SEC, duration, MIN_SAVINGS_PCT */
  int motion[2];
  unsigned long long segments[2];
  for (int i = 0; i < 2; ++i) {                    /* once without the boxes, once with them */
    uint8_t kept[F];
    double ts[F];
    uint64_t n = 0;
    CHECK(mtgpu_persist_flags(ctx, g_flags, g_has_sd, i ? g_box : NULL, F, stream_off, 1, MIN_RUN, 0, REACH, kept, NULL, NULL));
    for (int f = 0; f < F; ++f)
      if (kept[f]) ts[n++] = g_pts[f];
    mt_segment seg[F + 1];
    mt_merge_result res;
    CHECK(mtgpu_merge_segments(ctx, ts, n, &mp, 1, seg, F + 1, &res));
    motion[i] = (int)n;
    segments[i] = (unsigned long long)res.n_segments;
  }
  printf("MIN_RUN %d without boxes:       motion frames %d, segments %llu\n", MIN_RUN, motion[0], segments[0]);
  printf("MIN_RUN %d with boxes, reach %d: motion frames %d, segments %llu\n", MIN_RUN, REACH, motion[1], segments[1]);
  mtgpu_destroy(ctx);
  return 0;
}
