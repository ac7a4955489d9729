/* abi_tracks_canaries.c — the caller-sized buffers of include/mtgpu_tracks.h, allocated EXACTLY as the header states,
 * each with a canary region behind it that must be untouched after the call; every MT_ERR_INVALID of
 * mtgpu_track_objects_device with the argument named, nothing written and nothing taken from the context's scratch ring.
 * Plain C, HIP runtime API only for device memory; built and run by tests/test_gpu_tracks.py (-m gpu), built by
 * tests/test_tracks_host.py.
 *
 *   gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude tests/c/abi_tracks_canaries.c \
 *       -Lmotion-estimated-video-trimmer_amd -lmtgpu -L/opt/rocm/lib -lamdhip64
 */
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mtgpu.h"

#define CANARY 4096u           /* bytes behind every buffer */
#define PATTERN 0xA5
#define FILL 0x5A              /* what an output holds before a call */
#define FILL32 0x5A5A5A5Au

static int failures = 0;

#define MT(call)                                                                   \
  do {                                                                             \
    int rc_ = (call);                                                              \
    if (rc_ != MT_OK) {                                                            \
      fprintf(stderr, "%s:%d %s -> %d: %s\n", __FILE__, __LINE__, #call, rc_, mtgpu_last_error()); \
      exit(2);                                                                     \
    }                                                                              \
  } while (0)
#define HIP(call)                                                                  \
  do {                                                                             \
    hipError_t e_ = (call);                                                        \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "%s:%d %s -> %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
      exit(2);                                                                     \
    }                                                                              \
  } while (0)

/* device buffer of `bytes` USABLE bytes, the canary right behind them */
typedef struct dbuf { unsigned char *p; size_t bytes; const char *what; } dbuf;

static dbuf dalloc(size_t bytes, const char *what) {
  dbuf b = {NULL, bytes, what};
  HIP(hipMalloc((void **)&b.p, bytes + CANARY));
  HIP(hipMemset(b.p, FILL, bytes));
  HIP(hipMemset(b.p + bytes, PATTERN, CANARY));
  return b;
}

static void canary_check(const dbuf *b, const char *call) {
  static unsigned char host[CANARY];
  HIP(hipMemcpy(host, b->p + b->bytes, CANARY, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < CANARY; ++i)
    if (host[i] != PATTERN) {
      fprintf(stderr, "FAIL %s: %s (%zu bytes as the header sizes it) was overrun: canary byte %zu = 0x%02x\n", call, b->what,
              b->bytes, i, host[i]);
      ++failures;
      return;
    }
}

/* every usable byte still holds FILL */
static void untouched(const dbuf *b, const char *call) {
  unsigned char *host = malloc(b->bytes);
  if (!host) exit(2);
  HIP(hipMemcpy(host, b->p, b->bytes, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < b->bytes; ++i)
    if (host[i] != FILL) {
      fprintf(stderr, "FAIL %s: %s was written (byte %zu = 0x%02x)\n", call, b->what, i, host[i]);
      ++failures;
      break;
    }
  free(host);
}

static uint64_t reserved(mtgpu_ctx *ctx) {
  mtgpu_ctx_stats st;
  MT(mtgpu_get_stats(ctx, &st));
  return st.pool_reserved_bytes;
}

enum { K = 3 };

typedef struct args {
  const uint8_t *fl; const mt_object *li; int32_t k; uint32_t n; const uint64_t *so; uint32_t ns, reach; uint32_t *work;
  uint8_t *pred; uint32_t *age, *id, *len, *track; uint8_t *out;
} args;

static int call(mtgpu_ctx *ctx, const args *a) {
  return mtgpu_track_objects_device(ctx, a->fl, NULL, a->li, a->k, a->n, a->so, a->ns, 1, 0, a->reach, 2, a->work, a->pred, a->age, a->id,
                                    a->len, a->track, a->out, NULL);
}

int main(void) {
  mt_scan_params p;
  MT(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 2, 8, 0.05f));
  mtgpu_ctx *ctx = NULL;
  MT(mtgpu_create(&p, 0, &ctx));
  mtgpu_tracks_plan plan;
  MT(mtgpu_tracks_preview(K, &plan));
  const uint32_t T = (uint32_t)plan.frames_per_tile, n = 2 * T + 5;
  const size_t nk = (size_t)n * K;
  /* two frames in front of the streams, one behind; an empty stream in the middle */
  const uint64_t soff[4] = {2, T + 3, T + 3, n - 1};

  dbuf flags = dalloc(n, "d_flags"), list = dalloc(nk * sizeof(mt_object), "d_list"), so = dalloc(sizeof soff, "d_stream_off"),
       work = dalloc(nk * 4 * (size_t)plan.work_words_per_entry, "d_work"), pred = dalloc(nk, "d_pred"), age = dalloc(nk * 4, "d_age"),
       id = dalloc(nk * 4, "d_id"), len = dalloc(nk * 4, "d_len"), track = dalloc((size_t)n * 4, "d_track"), out = dalloc(n, "d_flags_out");
  dbuf *all[10] = {&flags, &list, &so, &work, &pred, &age, &id, &len, &track, &out};
  dbuf *outs[7] = {&work, &pred, &age, &id, &len, &track, &out};
  /* every frame is a motion frame; entry 0 is one cell at (0, 0) in every frame: one track per stream; entries 1, 2 are empty */
  mt_object *h_list = malloc(nk * sizeof(mt_object));
  if (!h_list) return 2;
  for (size_t e = 0; e < nk; ++e) {
    const mt_object one = {1, 0, 0, 0, 0, 0}, none = {0, 0xFFFFFFFFu, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF};
    h_list[e] = e % K == 0 ? one : none;
  }
  HIP(hipMemset(flags.p, 1, n));
  HIP(hipMemcpy(list.p, h_list, nk * sizeof(mt_object), hipMemcpyHostToDevice));
  HIP(hipMemcpy(so.p, soff, sizeof soff, hipMemcpyHostToDevice));
  const uint64_t before = reserved(ctx);

  /* ---- every refusal: the argument is named, no output byte changes, the canaries stand */
  unsigned char *host_words = malloc(nk * 4);
  if (!host_words) return 2;
  const args good = {flags.p, (const mt_object *)list.p, K, n, (const uint64_t *)so.p, 3, 1, (uint32_t *)work.p, pred.p, (uint32_t *)age.p,
                     (uint32_t *)id.p, (uint32_t *)len.p, (uint32_t *)track.p, out.p};
  struct { const char *name, *word; args a; } bad[20];
  int nb = 0;
#define BAD(NAME, WORD, EDIT)          \
  do {                                 \
    args a = good;                     \
    EDIT;                              \
    bad[nb].name = NAME;               \
    bad[nb].word = WORD;               \
    bad[nb++].a = a;                   \
  } while (0)
  BAD("all outputs NULL", "all NULL", (a.pred = NULL, a.age = a.id = a.len = a.track = NULL, a.out = NULL));
  BAD("k 0", "k is 0", a.k = 0);
  BAD("k 17", "k is 17", a.k = 17);
  BAD("n_frames x k at the limit", "not below 4294967295", (a.n = 0xFFFFFFFFu / 3u, a.k = 3));
  BAD("reach 65536", "reach", a.reach = 65536);
  BAD("d_flags NULL", "d_flags is NULL", a.fl = NULL);
  BAD("d_list NULL", "d_list is NULL", a.li = NULL);
  BAD("d_stream_off NULL", "d_stream_off is NULL", a.so = NULL);
  BAD("d_work NULL", "d_work is NULL", a.work = NULL);
  BAD("n_streams 0", "n_streams", a.ns = 0);
  BAD("d_list misaligned", "d_list must be 16-byte aligned", a.li = (const mt_object *)(list.p + 8));
  BAD("d_len misaligned", "d_len must be 4-byte aligned", a.len = (uint32_t *)(len.p + 2));
  BAD("d_track in host memory", "d_track is not memory of device", a.track = (uint32_t *)host_words);
  BAD("d_work in host memory", "d_work is not memory of device", a.work = (uint32_t *)host_words);
  BAD("d_flags_out is d_flags", "d_flags_out overlaps d_flags", a.out = (uint8_t *)flags.p);
  BAD("d_pred inside d_list", "d_pred overlaps d_list", a.pred = list.p + 16);
  BAD("d_id inside d_age", "d_id overlaps d_age", a.id = (uint32_t *)(age.p + 4));
  BAD("d_len is d_work's second half", "d_len overlaps d_work", a.len = (uint32_t *)(work.p + 4 * nk));
  for (int i = 0; i < nb; ++i) {
    memset(host_words, FILL, nk * 4);
    const int rc = call(ctx, &bad[i].a);
    if (rc != MT_ERR_INVALID || !strstr(mtgpu_last_error(), bad[i].word)) {
      fprintf(stderr, "FAIL %s: rc %d, \"%s\" (want MT_ERR_INVALID naming \"%s\")\n", bad[i].name, rc, mtgpu_last_error(), bad[i].word);
      ++failures;
    }
    HIP(hipDeviceSynchronize());
    for (int b = 0; b < 7; ++b) untouched(outs[b], bad[i].name);
    for (size_t k = 0; k < nk * 4; ++k)
      if (host_words[k] != FILL) {
        fprintf(stderr, "FAIL %s: the host buffer was written\n", bad[i].name);
        ++failures;
        break;
      }
    for (int b = 0; b < 10; ++b) canary_check(all[b], bad[i].name);
  }
  /* n_frames == 0: MT_OK, and nothing is touched */
  MT(mtgpu_track_objects_device(ctx, NULL, NULL, NULL, K, 0, NULL, 0, 1, 0, 1, 1, NULL, NULL, NULL, NULL, NULL, NULL, out.p, NULL));
  HIP(hipDeviceSynchronize());
  untouched(&out, "n_frames 0");

  /* ---- the call itself, every buffer at its stated size: all outputs, then each alone */
  uint8_t *h_pred = malloc(nk), *h_out = malloc(n);
  uint32_t *h_age = malloc(nk * 4), *h_id = malloc(nk * 4), *h_len = malloc(nk * 4), *h_track = malloc((size_t)n * 4);
  if (!h_pred || !h_out || !h_age || !h_id || !h_len || !h_track) return 2;
  for (int which = 0; which < 7; ++which) {
    for (int b = 0; b < 7; ++b) HIP(hipMemset(outs[b]->p, FILL, outs[b]->bytes));
    args a = good;
    if (which && which != 1) a.pred = NULL;
    if (which && which != 2) a.age = NULL;
    if (which && which != 3) a.id = NULL;
    if (which && which != 4) a.len = NULL;
    if (which && which != 5) a.track = NULL;
    if (which && which != 6) a.out = NULL;
    MT(mtgpu_track_objects_device(ctx, a.fl, NULL, a.li, K, n, a.so, 3, 1, 0, 0, T + 1, a.work, a.pred, a.age, a.id, a.len, a.track, a.out, NULL));
    HIP(hipDeviceSynchronize());
    HIP(hipMemcpy(h_pred, pred.p, nk, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(h_age, age.p, nk * 4, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(h_id, id.p, nk * 4, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(h_len, len.p, nk * 4, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(h_track, track.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(h_out, out.p, n, hipMemcpyDeviceToHost));
    for (uint32_t f = 0; f < n && !failures; ++f) {
      /* stream 0 has T + 1 frames, stream 2 has T + 1 too: n - 1 - (T + 3); each is one track of entry 0 */
      const int in0 = f >= soff[0] && f < soff[1], in2 = f >= soff[2] && f < soff[3];
      const uint32_t first = in0 ? (uint32_t)soff[0] : (uint32_t)soff[2];
      const uint32_t w_len = in0 || in2 ? T + 1 : 0, w_age = in0 || in2 ? f - first + 1 : 0;
      const uint32_t w_id = in0 || in2 ? first * K : MT_TRACK_NO_ID;
      const uint8_t w_pred = (in0 || in2) && f != first ? 0 : MT_TRACK_NO_PRED;
      for (uint32_t j = 0; j < K; ++j) {
        const size_t e = (size_t)f * K + j;
        const int ok = (a.pred ? h_pred[e] == (j ? MT_TRACK_NO_PRED : w_pred) : h_pred[e] == FILL) &&
                       (a.age ? h_age[e] == (j ? 0 : w_age) : h_age[e] == FILL32) &&
                       (a.id ? h_id[e] == (j ? MT_TRACK_NO_ID : w_id) : h_id[e] == FILL32) &&
                       (a.len ? h_len[e] == (j ? 0 : w_len) : h_len[e] == FILL32);
        if (!ok) {
          fprintf(stderr, "FAIL outputs %d: frame %u entry %u reads pred %u age %u id %u len %u\n", which, f, j, h_pred[e], h_age[e], h_id[e], h_len[e]);
          ++failures;
          break;
        }
      }
      if (!((a.track ? h_track[f] == w_len : h_track[f] == FILL32) && (a.out ? h_out[f] == (w_len >= T + 1) : h_out[f] == FILL))) {
        fprintf(stderr, "FAIL outputs %d: frame %u reads track %u flags_out %u\n", which, f, h_track[f], h_out[f]);
        ++failures;
      }
    }
    for (int b = 0; b < 10; ++b) canary_check(all[b], "mtgpu_track_objects_device");
  }
  if (reserved(ctx) != before) {
    fprintf(stderr, "FAIL: pool_reserved_bytes moved from %llu to %llu\n", (unsigned long long)before, (unsigned long long)reserved(ctx));
    ++failures;
  }

  for (int b = 0; b < 10; ++b) HIP(hipFree(all[b]->p));
  free(host_words);
  free(h_list);
  free(h_pred);
  free(h_out);
  free(h_age);
  free(h_id);
  free(h_len);
  free(h_track);
  mtgpu_destroy(ctx);
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  printf("all tracks buffers respected\n");
  return 0;
}
