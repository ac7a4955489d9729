/* abi_dir_canaries.c — the caller-sized buffers of include/mtgpu_dir.h, allocated EXACTLY as the header states, each with
 * a canary region behind it that must be untouched after the call; every MT_ERR_INVALID of mtgpu_scan_dir_device with
 * the argument named and nothing written.  Plain C, HIP runtime API only for device memory; built and run by
 * tests/test_gpu_dir.py (-m gpu), built by tests/test_dir_host.py.
 *
 *   gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude tests/c/abi_dir_canaries.c \
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

enum { F = 37, PER = 6 };      /* frames; records per frame */

int main(void) {
  mt_scan_params p;
  MT(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 1, 1, 0.0f));
  mtgpu_ctx *ctx = NULL;
  MT(mtgpu_create(&p, 0, &ctx));
  mtgpu_dir_plan plan;
  MT(mtgpu_dir_preview(&p, 163840, &plan));
  if (plan.rose_bytes != (int)sizeof(mt_dir_rose) || plan.sectors != 8) {
    fprintf(stderr, "FAIL: the plan says %d sectors, %d bytes per rose\n", plan.sectors, plan.rose_bytes);
    return 1;
  }

  /* every frame: three cells in a row whose records move east, three below that move west.  Two frames in front of
   * the streams, one behind; an empty stream in the middle.  Stream 0 allows E, stream 2 allows W. */
  mt_mv_compact rec[F * PER];
  uint64_t off[F + 1];
  for (int f = 0; f <= F; ++f) off[f] = (uint64_t)f * PER;
  for (int f = 0; f < F; ++f)
    for (int j = 0; j < PER; ++j) {
      mt_mv_compact *v = &rec[f * PER + j];
      const int east = j < 3;
      v->dst_x = (int16_t)(16 * (20 + j % 3) + 8);
      v->dst_y = (int16_t)(16 * (east ? 10 : 20) + 8);
      v->src_x = (int16_t)(v->dst_x - (east ? 6 : -6));
      v->src_y = v->dst_y;
    }
  const uint64_t soff[4] = {2, 20, 20, F - 1};
  const uint8_t allows[3] = {0x01, 0xFF, 0x10};

  dbuf d_rec = dalloc(sizeof rec, "d_rec"), d_off = dalloc(sizeof off, "d_frame_off"), d_so = dalloc(sizeof soff, "d_stream_off"),
       d_al = dalloc(sizeof allows, "d_allow"), fl = dalloc(F, "d_flags"), ce = dalloc((size_t)F * 4, "d_centres"),
       ro = dalloc((size_t)F * sizeof(mt_dir_rose), "d_rose");
  dbuf *all[7] = {&d_rec, &d_off, &d_so, &d_al, &fl, &ce, &ro};
  HIP(hipMemcpy(d_rec.p, rec, sizeof rec, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_off.p, off, sizeof off, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_so.p, soff, sizeof soff, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_al.p, allows, sizeof allows, hipMemcpyHostToDevice));

  /* ---- every refusal: the argument is named, no output byte changes, the canaries stand */
  unsigned char *host_out = malloc((size_t)F * sizeof(mt_dir_rose));
  if (!host_out) return 2;
  struct {
    const char *name, *word;
    int rec_bytes; const uint64_t *off, *so; uint32_t ns; const uint8_t *al; int32_t allow; uint8_t *fl; uint32_t *ce; mt_dir_rose *ro;
  } bad[] = {
      {"allow 256", "allow", 8, (uint64_t *)d_off.p, (uint64_t *)d_so.p, 3, d_al.p, 256, fl.p, (uint32_t *)ce.p, (mt_dir_rose *)ro.p},
      {"allow -1", "allow", 8, (uint64_t *)d_off.p, NULL, 0, NULL, -1, fl.p, (uint32_t *)ce.p, (mt_dir_rose *)ro.p},
      {"rec_bytes 16", "rec_bytes", 16, (uint64_t *)d_off.p, NULL, 0, NULL, 255, fl.p, (uint32_t *)ce.p, (mt_dir_rose *)ro.p},
      {"all outputs NULL", "all NULL", 8, (uint64_t *)d_off.p, NULL, 0, NULL, 255, NULL, NULL, NULL},
      {"d_frame_off NULL", "d_frame_off", 8, NULL, NULL, 0, NULL, 255, fl.p, (uint32_t *)ce.p, (mt_dir_rose *)ro.p},
      {"d_allow without d_stream_off", "d_stream_off", 8, (uint64_t *)d_off.p, NULL, 3, d_al.p, 255, fl.p, (uint32_t *)ce.p,
       (mt_dir_rose *)ro.p},
      {"d_allow without n_streams", "n_streams", 8, (uint64_t *)d_off.p, (uint64_t *)d_so.p, 0, d_al.p, 255, fl.p, (uint32_t *)ce.p,
       (mt_dir_rose *)ro.p},
      {"d_stream_off without d_allow", "d_allow", 8, (uint64_t *)d_off.p, (uint64_t *)d_so.p, 0, NULL, 255, fl.p, (uint32_t *)ce.p,
       (mt_dir_rose *)ro.p},
      {"n_streams without d_allow", "d_allow", 8, (uint64_t *)d_off.p, NULL, 3, NULL, 255, fl.p, (uint32_t *)ce.p, (mt_dir_rose *)ro.p},
      {"d_frame_off misaligned", "d_frame_off", 8, (uint64_t *)(d_off.p + 4), NULL, 0, NULL, 255, fl.p, (uint32_t *)ce.p,
       (mt_dir_rose *)ro.p},
      {"d_rose misaligned", "d_rose", 8, (uint64_t *)d_off.p, NULL, 0, NULL, 255, fl.p, (uint32_t *)ce.p, (mt_dir_rose *)(ro.p + 2)},
      {"d_centres misaligned", "d_centres", 8, (uint64_t *)d_off.p, NULL, 0, NULL, 255, fl.p, (uint32_t *)(ce.p + 1), (mt_dir_rose *)ro.p},
      {"d_rose in host memory", "d_rose is not memory of device", 8, (uint64_t *)d_off.p, NULL, 0, NULL, 255, fl.p, (uint32_t *)ce.p,
       (mt_dir_rose *)host_out},
      {"d_flags in host memory", "d_flags is not memory of device", 8, (uint64_t *)d_off.p, NULL, 0, NULL, 255, host_out, (uint32_t *)ce.p,
       (mt_dir_rose *)ro.p},
  };
  for (size_t i = 0; i < sizeof bad / sizeof bad[0]; ++i) {
    memset(host_out, FILL, (size_t)F * sizeof(mt_dir_rose));
    const int rc = mtgpu_scan_dir_device(ctx, d_rec.p, bad[i].rec_bytes, (uint64_t)F * PER, bad[i].off, NULL, F, bad[i].so, bad[i].ns,
                                         bad[i].al, bad[i].allow, bad[i].fl, bad[i].ce, bad[i].ro, NULL);
    if (rc != MT_ERR_INVALID || !strstr(mtgpu_last_error(), bad[i].word)) {
      fprintf(stderr, "FAIL %s: rc %d, \"%s\" (want MT_ERR_INVALID naming \"%s\")\n", bad[i].name, rc, mtgpu_last_error(), bad[i].word);
      ++failures;
    }
    HIP(hipDeviceSynchronize());
    untouched(&fl, bad[i].name);
    untouched(&ce, bad[i].name);
    untouched(&ro, bad[i].name);
    for (size_t k = 0; k < (size_t)F * sizeof(mt_dir_rose); ++k)
      if (host_out[k] != FILL) {
        fprintf(stderr, "FAIL %s: the host buffer was written\n", bad[i].name);
        ++failures;
        break;
      }
    for (int b = 0; b < 7; ++b) canary_check(all[b], bad[i].name);
  }
  /* n_frames == 0: MT_OK, and nothing is touched */
  MT(mtgpu_scan_dir_device(ctx, NULL, 8, 0, NULL, NULL, 0, NULL, 0, NULL, 255, fl.p, (uint32_t *)ce.p, (mt_dir_rose *)ro.p, NULL));
  HIP(hipDeviceSynchronize());
  untouched(&fl, "n_frames 0");
  untouched(&ce, "n_frames 0");
  untouched(&ro, "n_frames 0");

  /* ---- the call itself, every buffer at its stated size: all outputs, then each alone; with streams, then the scalar */
  uint8_t h_fl[F];
  uint32_t h_ce[F];
  mt_dir_rose h_ro[F];
  for (int form = 0; form < 2; ++form)
    for (int which = 0; which < 4; ++which) {
      HIP(hipMemset(fl.p, FILL, fl.bytes));
      HIP(hipMemset(ce.p, FILL, ce.bytes));
      HIP(hipMemset(ro.p, FILL, ro.bytes));
      uint8_t *a = which == 0 || which == 1 ? fl.p : NULL;
      uint32_t *b = which == 0 || which == 2 ? (uint32_t *)ce.p : NULL;
      mt_dir_rose *c = which == 0 || which == 3 ? (mt_dir_rose *)ro.p : NULL;
      if (form == 0)
        MT(mtgpu_scan_dir_device(ctx, d_rec.p, 8, (uint64_t)F * PER, (uint64_t *)d_off.p, NULL, F, (uint64_t *)d_so.p, 3, d_al.p, 0, a, b, c,
                                 NULL));
      else
        MT(mtgpu_scan_dir_device(ctx, d_rec.p, 8, (uint64_t)F * PER, (uint64_t *)d_off.p, NULL, F, NULL, 0, NULL, 0x10, a, b, c, NULL));
      HIP(hipDeviceSynchronize());
      HIP(hipMemcpy(h_fl, fl.p, sizeof h_fl, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_ce, ce.p, sizeof h_ce, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_ro, ro.p, sizeof h_ro, hipMemcpyDeviceToHost));
      for (uint32_t f = 0; f < F; ++f) {
        /* three cells in a row: 3 centres per allowed direction; a frame outside the streams reads 0 */
        const int live = form == 1 || (f >= soff[0] && f < soff[3]);
        const uint32_t want_c = live ? 3u : 0u, want_e = live ? 3u : 0u, want_w = want_e;
        int ok = (a ? h_fl[f] == (want_c >= 1) : h_fl[f] == FILL) && (b ? h_ce[f] == want_c : h_ce[f] == 0x5A5A5A5Au);
        for (int k = 0; k < 8; ++k)
          ok = ok && (c ? h_ro[f].n[k] == (k == 0 ? want_e : k == 4 ? want_w : 0u) : h_ro[f].n[k] == 0x5A5A5A5Au);
        if (!ok) {
          fprintf(stderr, "FAIL form %d outputs %d: frame %u reads flag %u centres %u rose E %u W %u\n", form, which, f, h_fl[f], h_ce[f],
                  h_ro[f].n[0], h_ro[f].n[4]);
          ++failures;
          break;
        }
      }
      for (int k = 0; k < 7; ++k) canary_check(all[k], "mtgpu_scan_dir_device");
    }

  for (int k = 0; k < 7; ++k) HIP(hipFree(all[k]->p));
  free(host_out);
  mtgpu_destroy(ctx);
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  printf("all direction buffers respected\n");
  return 0;
}
