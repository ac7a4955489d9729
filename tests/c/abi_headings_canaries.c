/* abi_headings_canaries.c — the caller-sized buffers of include/mtgpu_headings.h, allocated EXACTLY as the header states,
 * each with a canary region behind it that must be untouched after the call; every MT_ERR_INVALID of
 * mtgpu_scan_headings_device with the argument named and nothing written.  Plain C, HIP runtime API only for device
 * memory; built and run by tests/test_gpu_headings.py (-m gpu), built by tests/test_headings_host.py.
 *
 *   gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude tests/c/abi_headings_canaries.c \
 *       -Lmotion-estimated-video-trimmer_amd -lmtgpu -L/opt/rocm/lib -lamdhip64
 */
#include <hip/hip_runtime_api.h>
#include <stddef.h>
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

typedef char heading_is_64_bytes[sizeof(mt_heading) == 64 && offsetof(mt_heading, records) == 32 && offsetof(mt_heading, heading) == 36 &&
                                         offsetof(mt_heading, sum_dx) == 40 && offsetof(mt_heading, sum_dy) == 48 &&
                                         offsetof(mt_heading, reserved) == 56
                                     ? 1
                                     : -1];

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

enum { F = 37, PER = 5, K = 4, GW = 120, GH = 68, W = 2, NOUT = 7, NBUF = 11 };   /* frames; records per frame; entries; the 1080p grid */

int main(void) {
  mt_scan_params p;
  MT(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 1, 1, 0.0f));
  mtgpu_ctx *ctx = NULL;
  MT(mtgpu_create(&p, 0, &ctx));
  mtgpu_headings_plan plan;
  mtgpu_objects_plan oplan;
  MT(mtgpu_headings_preview(&p, K, 163840, &plan));
  MT(mtgpu_objects_preview(&p, K, 163840, &oplan));
  if (plan.lds_bytes != oplan.lds_bytes + K * MT_HEADING_TABLE_BYTES || plan.keep_words_per_stream != GH * W) {
    fprintf(stderr, "FAIL: the plan says %d bytes of LDS (objects: %d), %d keep words per stream\n", plan.lds_bytes, oplan.lds_bytes,
            plan.keep_words_per_stream);
    return 1;
  }

  /* every frame: a run of three cells on row 10 moving E by 6 and a run of two on row 20 moving N by 7, both from column
   * 20.  Two frames in front of the streams (they take plane 0), one behind; an empty stream in the middle; all planes
   * keep everything. */
  mt_mv_compact rec[F * PER];
  uint64_t off[F + 1];
  for (int f = 0; f <= F; ++f) off[f] = (uint64_t)f * PER;
  for (int f = 0; f < F; ++f)
    for (int j = 0; j < PER; ++j) {
      mt_mv_compact *v = &rec[f * PER + j];
      const int three = j < 3;
      v->dst_x = (int16_t)(16 * (20 + (three ? j : j - 3)) + 8);
      v->dst_y = (int16_t)(16 * (three ? 10 : 20) + 8);
      v->src_x = (int16_t)(v->dst_x - (three ? 6 : 0));
      v->src_y = (int16_t)(v->dst_y + (three ? 0 : 7));
    }
  const uint64_t soff[4] = {2, 20, 20, F - 1};
  static uint64_t keep[3 * GH * W];
  memset(keep, 0xFF, sizeof keep);

  dbuf d_rec = dalloc(sizeof rec, "d_rec"), d_off = dalloc(sizeof off, "d_frame_off"), d_so = dalloc(sizeof soff, "d_stream_off"),
       d_kp = dalloc(sizeof keep, "d_keep"), fl = dalloc(F, "d_flags"), ce = dalloc((size_t)F * 4, "d_centres"),
       bl = dalloc((size_t)F * 4, "d_blobs"), ob = dalloc((size_t)F * 4, "d_objects"), li = dalloc((size_t)F * K * sizeof(mt_object), "d_list"),
       mo = dalloc((size_t)F * K * sizeof(mt_heading), "d_motion"), al = dalloc((size_t)F * 4, "d_allowed");
  dbuf *all[NBUF] = {&d_rec, &d_off, &d_so, &d_kp, &fl, &ce, &bl, &ob, &li, &mo, &al};
  dbuf *outs[NOUT] = {&fl, &ce, &bl, &ob, &li, &mo, &al};
  HIP(hipMemcpy(d_rec.p, rec, sizeof rec, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_off.p, off, sizeof off, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_so.p, soff, sizeof soff, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_kp.p, keep, sizeof keep, hipMemcpyHostToDevice));

  /* ---- every refusal: the argument is named, no output byte changes, the canaries stand */
  const size_t host_bytes = (size_t)F * K * sizeof(mt_heading);
  unsigned char *host_out = malloc(host_bytes);
  if (!host_out) return 2;
  uint64_t *OFF = (uint64_t *)d_off.p, *SO = (uint64_t *)d_so.p, *KP = (uint64_t *)d_kp.p;
  uint32_t *CE = (uint32_t *)ce.p, *BL = (uint32_t *)bl.p, *OB = (uint32_t *)ob.p, *AL = (uint32_t *)al.p;
  mt_object *LI = (mt_object *)li.p;
  mt_heading *MO = (mt_heading *)mo.p;
  struct {
    const char *name, *word;
    int32_t k, min_objects, allow; int rec_bytes; const uint64_t *off, *so; uint32_t ns; const uint64_t *kp; uint8_t *fl; uint32_t *ce, *bl, *ob;
    mt_object *li; mt_heading *mo; uint32_t *al;
  } bad[] = {
      {"k 0", "k is 0", 0, 1, 255, 8, OFF, NULL, 0, NULL, fl.p, CE, BL, OB, LI, MO, AL},
      {"k 17", "k is 17", 17, 1, 255, 8, OFF, NULL, 0, NULL, fl.p, CE, BL, OB, LI, MO, AL},
      {"min_objects above k", "min_objects is 5, above k = 4", K, 5, 255, 8, OFF, NULL, 0, NULL, fl.p, CE, BL, OB, LI, MO, AL},
      {"allow 256", "allow 256", K, 1, 256, 8, OFF, NULL, 0, NULL, fl.p, CE, BL, OB, LI, MO, AL},
      {"allow -1", "allow -1", K, 1, -1, 8, OFF, SO, 3, KP, fl.p, CE, BL, OB, LI, MO, AL},
      {"rec_bytes 16", "rec_bytes", K, 1, 255, 16, OFF, NULL, 0, NULL, fl.p, CE, BL, OB, LI, MO, AL},
      {"all outputs NULL", "all NULL", K, 1, 255, 8, OFF, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL},
      {"d_frame_off NULL", "d_frame_off", K, 1, 255, 8, NULL, NULL, 0, NULL, fl.p, CE, BL, OB, LI, MO, AL},
      {"d_keep without d_stream_off", "d_stream_off", K, 1, 255, 8, OFF, NULL, 3, KP, fl.p, CE, BL, OB, LI, MO, AL},
      {"d_keep without n_streams", "n_streams", K, 1, 255, 8, OFF, SO, 0, KP, fl.p, CE, BL, OB, LI, MO, AL},
      {"d_stream_off without d_keep", "d_keep", K, 1, 255, 8, OFF, SO, 0, NULL, fl.p, CE, BL, OB, LI, MO, AL},
      {"d_frame_off misaligned", "d_frame_off", K, 1, 255, 8, (uint64_t *)(d_off.p + 4), NULL, 0, NULL, fl.p, CE, BL, OB, LI, MO, AL},
      {"d_motion misaligned by 8", "d_motion must be 16-byte aligned", K, 1, 255, 8, OFF, NULL, 0, NULL, fl.p, CE, BL, OB, LI,
       (mt_heading *)(mo.p + 8), AL},
      {"d_motion misaligned by 4", "d_motion must be 16-byte aligned", K, 1, 255, 8, OFF, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL,
       (mt_heading *)(mo.p + 4), NULL},
      {"d_list misaligned by 8", "d_list must be 16-byte aligned", K, 1, 255, 8, OFF, NULL, 0, NULL, fl.p, CE, BL, OB, (mt_object *)(li.p + 8), MO, AL},
      {"d_allowed misaligned", "d_allowed", K, 1, 255, 8, OFF, NULL, 0, NULL, fl.p, CE, BL, OB, LI, MO, (uint32_t *)(al.p + 2)},
      {"d_motion in host memory", "d_motion is not memory of device", K, 1, 255, 8, OFF, NULL, 0, NULL, fl.p, CE, BL, OB, LI,
       (mt_heading *)host_out, AL},
      {"d_allowed in host memory", "d_allowed is not memory of device", K, 1, 255, 8, OFF, NULL, 0, NULL, fl.p, CE, BL, OB, LI, MO,
       (uint32_t *)host_out},
  };
  for (size_t i = 0; i < sizeof bad / sizeof bad[0]; ++i) {
    memset(host_out, FILL, host_bytes);
    const int rc = mtgpu_scan_headings_device(ctx, d_rec.p, bad[i].rec_bytes, (uint64_t)F * PER, bad[i].off, NULL, F, bad[i].so, bad[i].ns,
                                              bad[i].kp, bad[i].k, 1, bad[i].min_objects, bad[i].allow, bad[i].fl, bad[i].ce, bad[i].bl,
                                              bad[i].ob, bad[i].li, bad[i].mo, bad[i].al, NULL);
    if (rc != MT_ERR_INVALID || !strstr(mtgpu_last_error(), bad[i].word)) {
      fprintf(stderr, "FAIL %s: rc %d, \"%s\" (want MT_ERR_INVALID naming \"%s\")\n", bad[i].name, rc, mtgpu_last_error(), bad[i].word);
      ++failures;
    }
    HIP(hipDeviceSynchronize());
    for (int b = 0; b < NOUT; ++b) untouched(outs[b], bad[i].name);
    for (size_t k = 0; k < host_bytes; ++k)
      if (host_out[k] != FILL) {
        fprintf(stderr, "FAIL %s: the host buffer was written\n", bad[i].name);
        ++failures;
        break;
      }
    for (int b = 0; b < NBUF; ++b) canary_check(all[b], bad[i].name);
  }
  /* n_frames == 0: MT_OK, and nothing is touched */
  MT(mtgpu_scan_headings_device(ctx, NULL, 8, 0, NULL, NULL, 0, NULL, 0, NULL, K, 1, 1, 255, fl.p, CE, BL, OB, LI, MO, AL, NULL));
  HIP(hipDeviceSynchronize());
  for (int b = 0; b < NOUT; ++b) untouched(outs[b], "n_frames 0");

  /* ---- the call itself, every buffer at its stated size: all outputs, then each alone; with streams, then without.
   * min_blob_cells 2, min_objects 1, every heading but N allowed: one allowed object per live frame. */
  uint8_t h_fl[F];
  uint32_t h_ce[F], h_al[F];
  static mt_object h_li[F * K];
  static mt_heading h_mo[F * K];
  mt_heading none, first, second, junk;
  memset(&none, 0, sizeof none);
  none.heading = MT_HEADING_NONE;
  first = none; first.n[0] = 3; first.records = 3; first.heading = 0; first.sum_dx = 18;
  second = none; second.n[6] = 2; second.records = 2; second.heading = 6; second.sum_dy = -14;
  memset(&junk, FILL, sizeof junk);
  for (int form = 0; form < 2; ++form)
    for (int which = 0; which <= NOUT; ++which) {
      for (int b = 0; b < NOUT; ++b) HIP(hipMemset(outs[b]->p, FILL, outs[b]->bytes));
#define WANT(i) (which == 0 || which == (i))
      MT(mtgpu_scan_headings_device(ctx, d_rec.p, 8, (uint64_t)F * PER, OFF, NULL, F, form == 0 ? SO : NULL, form == 0 ? 3 : 0,
                                    form == 0 ? KP : NULL, K, 2, 1, 0xFF & ~(1 << 6), WANT(1) ? fl.p : NULL, WANT(2) ? CE : NULL,
                                    WANT(3) ? BL : NULL, WANT(4) ? OB : NULL, WANT(5) ? LI : NULL, WANT(6) ? MO : NULL, WANT(7) ? AL : NULL,
                                    NULL));
      HIP(hipDeviceSynchronize());
      HIP(hipMemcpy(h_fl, fl.p, sizeof h_fl, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_ce, ce.p, sizeof h_ce, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_al, al.p, sizeof h_al, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_li, li.p, sizeof h_li, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_mo, mo.p, sizeof h_mo, hipMemcpyDeviceToHost));
      for (uint32_t f = 0; f < F; ++f) {
        /* a frame behind the last stream reads zeros and empty entries; one in front of the first takes plane 0 */
        const int live = form == 1 || f < soff[3];
        const uint32_t junk32 = 0x5A5A5A5Au;
        int ok = (WANT(1) ? h_fl[f] == (live ? 1 : 0) : h_fl[f] == FILL) && (WANT(2) ? h_ce[f] == (live ? 5u : 0u) : h_ce[f] == junk32) &&
                 (WANT(7) ? h_al[f] == (live ? 1u : 0u) : h_al[f] == junk32) &&
                 (WANT(5) ? h_li[f * K].cells == (live ? 3u : 0u) && h_li[f * K + 1].cells == (live ? 2u : 0u) && h_li[f * K + 2].cells == 0u
                          : h_li[f * K].cells == junk32);
        for (int j = 0; j < K; ++j) {
          const mt_heading *want = !WANT(6) ? &junk : live && j == 0 ? &first : live && j == 1 ? &second : &none;
          ok = ok && memcmp(&h_mo[f * K + j], want, sizeof *want) == 0;
        }
        if (!ok) {
          const mt_heading *g = &h_mo[f * K];
          fprintf(stderr, "FAIL form %d outputs %d: frame %u reads flag %u centres %u allowed %u, entry 0 {n0 %u, records %u, heading %u, "
                  "sum_dx %lld, sum_dy %lld}\n", form, which, f, h_fl[f], h_ce[f], h_al[f], g->n[0], g->records, g->heading,
                  (long long)g->sum_dx, (long long)g->sum_dy);
          ++failures;
          break;
        }
      }
      for (int k = 0; k < NBUF; ++k) canary_check(all[k], "mtgpu_scan_headings_device");
    }

  for (int k = 0; k < NBUF; ++k) HIP(hipFree(all[k]->p));
  free(host_out);
  mtgpu_destroy(ctx);
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  printf("all heading buffers respected\n");
  return 0;
}
