/* abi_persist_canaries.c — the caller-sized buffers of include/mtgpu_persist.h, allocated EXACTLY as the header states,
 * each with a canary region behind it that must be untouched after the call; every MT_ERR_INVALID of
 * mtgpu_persist_flags_device with the argument named, nothing written and nothing taken from the context's scratch ring.
 * Plain C, HIP runtime API only for device memory; built and run by tests/test_gpu_persist.py (-m gpu), built by
 * tests/test_persist_host.py.
 *
 *   gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude tests/c/abi_persist_canaries.c \
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

/* every usable byte still holds `value` */
static void untouched(const dbuf *b, int value, const char *call) {
  unsigned char *host = malloc(b->bytes);
  if (!host) exit(2);
  HIP(hipMemcpy(host, b->p, b->bytes, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < b->bytes; ++i)
    if (host[i] != (unsigned char)value) {
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

int main(void) {
  mt_scan_params p;
  MT(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 2, 8, 0.05f));
  mtgpu_ctx *ctx = NULL;
  MT(mtgpu_create(&p, 0, &ctx));
  mtgpu_persist_plan plan;
  MT(mtgpu_persist_preview(&plan));
  const uint32_t T = (uint32_t)plan.frames_per_tile, n = 2 * T + 5;
  /* two frames in front of the streams, one behind; an empty stream in the middle */
  const uint64_t soff[4] = {2, T + 3, T + 3, n - 1};

  dbuf flags = dalloc(n, "d_flags"), sd = dalloc(n, "d_has_sd"), box = dalloc((size_t)n * sizeof(mt_blob_box), "d_box"),
       so = dalloc(sizeof soff, "d_stream_off"), work = dalloc((size_t)n * 4, "d_work"), out = dalloc(n, "d_flags_out"),
       run = dalloc((size_t)n * 4, "d_run"), pos = dalloc((size_t)n * 4, "d_pos");
  dbuf *all[8] = {&flags, &sd, &box, &so, &work, &out, &run, &pos};
  HIP(hipMemset(flags.p, 1, n));                     /* every frame is a motion frame */
  HIP(hipMemset(sd.p, 1, n));
  HIP(hipMemset(box.p, 0, box.bytes));               /* every box is cell (0, 0): all linked */
  HIP(hipMemcpy(so.p, soff, sizeof soff, hipMemcpyHostToDevice));
  const uint64_t before = reserved(ctx);

  /* ---- every refusal: the argument is named, no output byte changes, the canaries stand */
  unsigned char *host_words = malloc((size_t)n * 4);
  if (!host_words) return 2;
  struct {
    const char *name, *word;
    const uint8_t *fl; const uint64_t *so; uint32_t ns, reach; uint32_t *work; uint8_t *out; uint32_t *run, *pos;
  } bad[] = {
      {"all outputs NULL", "all NULL", flags.p, (uint64_t *)so.p, 3, 1, (uint32_t *)work.p, NULL, NULL, NULL},
      {"d_flags NULL", "d_flags", NULL, (uint64_t *)so.p, 3, 1, (uint32_t *)work.p, out.p, (uint32_t *)run.p, (uint32_t *)pos.p},
      {"d_stream_off NULL", "d_stream_off", flags.p, NULL, 3, 1, (uint32_t *)work.p, out.p, (uint32_t *)run.p, (uint32_t *)pos.p},
      {"d_work NULL", "d_work", flags.p, (uint64_t *)so.p, 3, 1, NULL, out.p, (uint32_t *)run.p, (uint32_t *)pos.p},
      {"n_streams 0", "n_streams", flags.p, (uint64_t *)so.p, 0, 1, (uint32_t *)work.p, out.p, (uint32_t *)run.p, (uint32_t *)pos.p},
      {"reach 65536", "reach", flags.p, (uint64_t *)so.p, 3, 65536, (uint32_t *)work.p, out.p, (uint32_t *)run.p, (uint32_t *)pos.p},
      {"d_pos misaligned", "d_pos", flags.p, (uint64_t *)so.p, 3, 1, (uint32_t *)work.p, out.p, (uint32_t *)run.p, (uint32_t *)(pos.p + 2)},
      {"d_run in host memory", "d_run is not memory of device", flags.p, (uint64_t *)so.p, 3, 1, (uint32_t *)work.p, out.p,
       (uint32_t *)host_words, (uint32_t *)pos.p},
      {"d_work in host memory", "d_work is not memory of device", flags.p, (uint64_t *)so.p, 3, 1, (uint32_t *)host_words, out.p,
       (uint32_t *)run.p, (uint32_t *)pos.p},
      {"d_flags_out is d_flags", "d_flags_out overlaps d_flags", flags.p, (uint64_t *)so.p, 3, 1, (uint32_t *)work.p, flags.p,
       (uint32_t *)run.p, (uint32_t *)pos.p},
      {"d_pos inside d_run", "d_pos overlaps d_run", flags.p, (uint64_t *)so.p, 3, 1, (uint32_t *)work.p, out.p, (uint32_t *)run.p,
       (uint32_t *)(run.p + 4 * (size_t)(n - 1))},
      {"d_run is d_work", "d_run overlaps d_work", flags.p, (uint64_t *)so.p, 3, 1, (uint32_t *)work.p, out.p, (uint32_t *)work.p, NULL},
  };
  for (size_t i = 0; i < sizeof bad / sizeof bad[0]; ++i) {
    memset(host_words, FILL, (size_t)n * 4);
    const int rc = mtgpu_persist_flags_device(ctx, bad[i].fl, sd.p, (const mt_blob_box *)box.p, n, bad[i].so, bad[i].ns, 2, 0,
                                              bad[i].reach, bad[i].work, bad[i].out, bad[i].run, bad[i].pos, NULL);
    if (rc != MT_ERR_INVALID || !strstr(mtgpu_last_error(), bad[i].word)) {
      fprintf(stderr, "FAIL %s: rc %d, \"%s\" (want MT_ERR_INVALID naming \"%s\")\n", bad[i].name, rc, mtgpu_last_error(), bad[i].word);
      ++failures;
    }
    HIP(hipDeviceSynchronize());
    untouched(&flags, 1, bad[i].name);
    untouched(&work, FILL, bad[i].name);
    untouched(&out, FILL, bad[i].name);
    untouched(&run, FILL, bad[i].name);
    untouched(&pos, FILL, bad[i].name);
    for (size_t k = 0; k < (size_t)n * 4; ++k)
      if (host_words[k] != FILL) {
        fprintf(stderr, "FAIL %s: the host buffer was written\n", bad[i].name);
        ++failures;
        break;
      }
    for (int b = 0; b < 8; ++b) canary_check(all[b], bad[i].name);
  }
  /* n_frames == 0: MT_OK, and nothing is touched */
  MT(mtgpu_persist_flags_device(ctx, NULL, NULL, NULL, 0, NULL, 0, 1, 0, 1, NULL, out.p, NULL, NULL, NULL));
  HIP(hipDeviceSynchronize());
  untouched(&out, FILL, "n_frames 0");

  /* ---- the call itself, every buffer at its stated size: all outputs, then each alone */
  uint32_t *h_run = malloc((size_t)n * 4), *h_pos = malloc((size_t)n * 4);
  uint8_t *h_out = malloc(n);
  if (!h_run || !h_pos || !h_out) return 2;
  for (int which = 0; which < 4; ++which) {
    HIP(hipMemset(out.p, FILL, out.bytes));
    HIP(hipMemset(run.p, FILL, run.bytes));
    HIP(hipMemset(pos.p, FILL, pos.bytes));
    uint8_t *a = which == 0 || which == 1 ? out.p : NULL;
    uint32_t *b = which == 0 || which == 2 ? (uint32_t *)run.p : NULL, *c = which == 0 || which == 3 ? (uint32_t *)pos.p : NULL;
    MT(mtgpu_persist_flags_device(ctx, flags.p, sd.p, (const mt_blob_box *)box.p, n, (uint64_t *)so.p, 3, T + 1, 0, 0,
                                  (uint32_t *)work.p, a, b, c, NULL));
    HIP(hipDeviceSynchronize());
    HIP(hipMemcpy(h_out, out.p, n, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(h_run, run.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(h_pos, pos.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (uint32_t f = 0; f < n; ++f) {
      /* stream 0 has T + 1 frames (kept at min_run T + 1), stream 2 has T + 1 too: n - 1 - (T + 3) */
      const int in0 = f >= soff[0] && f < soff[1], in2 = f >= soff[2] && f < soff[3];
      const uint32_t want_run = in0 ? (uint32_t)(soff[1] - soff[0]) : in2 ? (uint32_t)(soff[3] - soff[2]) : 0;
      const uint32_t want_pos = in0 ? f - (uint32_t)soff[0] + 1 : in2 ? f - (uint32_t)soff[2] + 1 : 0;
      const uint8_t want_out = want_run >= T + 1;
      const int ok = (a ? h_out[f] == want_out : h_out[f] == FILL) && (b ? h_run[f] == want_run : h_run[f] == 0x5A5A5A5Au) &&
                     (c ? h_pos[f] == want_pos : h_pos[f] == 0x5A5A5A5Au);
      if (!ok) {
        fprintf(stderr, "FAIL outputs %d: frame %u reads flags_out %u run %u pos %u\n", which, f, h_out[f], h_run[f], h_pos[f]);
        ++failures;
        break;
      }
    }
    for (int k = 0; k < 8; ++k) canary_check(all[k], "mtgpu_persist_flags_device");
  }
  if (reserved(ctx) != before) {
    fprintf(stderr, "FAIL: pool_reserved_bytes moved from %llu to %llu\n", (unsigned long long)before, (unsigned long long)reserved(ctx));
    ++failures;
  }

  for (int k = 0; k < 8; ++k) HIP(hipFree(all[k]->p));
  free(host_words);
  free(h_run);
  free(h_pos);
  free(h_out);
  mtgpu_destroy(ctx);
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  printf("all persistence buffers respected\n");
  return 0;
}
