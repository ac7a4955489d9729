/* abi_lanes_canaries.c — the caller-sized buffers of include/mtgpu_lanes.h, allocated EXACTLY as the header states, each
 * with a canary region behind it that must be untouched after the call; every MT_ERR_INVALID of mtgpu_scan_lanes_device
 * and mtgpu_flow_map_device with the argument named and nothing written.  Plain C, HIP runtime API only for device
 * memory; built and run by tests/test_gpu_lanes.py (-m gpu), built by tests/test_lanes_host.py.
 *
 *   gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude tests/c/abi_lanes_canaries.c \
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

enum { F = 37, PER = 6, NS = 3 };      /* frames; records per frame; streams */

int main(void) {
  mt_scan_params p;
  MT(mtgpu_params_from_config(&p, 1920, 1080, 16.0, 16, 4, 1, 1, 0.0f));
  mtgpu_ctx *ctx = NULL;
  MT(mtgpu_create(&p, 0, &ctx));
  mtgpu_lanes_plan plan;
  MT(mtgpu_lanes_preview(&p, 163840, &plan));
  const size_t cells = (size_t)p.grid_w * (size_t)p.grid_h;
  if ((size_t)plan.plane_bytes != cells || plan.staged != 1) {
    fprintf(stderr, "FAIL: the plan says %d bytes per plane, staged %d\n", plan.plane_bytes, plan.staged);
    return 1;
  }

  /* every frame: three cells in row 10 whose records move east, three in row 20 that move west.  Two frames in front of
   * the streams, one behind; an empty stream in the middle.  Plane 0 allows E everywhere, plane 2 allows W everywhere. */
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
  const uint64_t soff[NS + 1] = {2, 20, 20, F - 1};
  uint8_t *planes = malloc(NS * cells);
  if (!planes) return 2;
  memset(planes, 0x01, cells);
  memset(planes + cells, 0xFF, cells);
  memset(planes + 2 * cells, 0x10, cells);
  const size_t flow_words = (size_t)NS * 8u * cells;

  dbuf d_rec = dalloc(sizeof rec, "d_rec"), d_off = dalloc(sizeof off, "d_frame_off"), d_so = dalloc(sizeof soff, "d_stream_off"),
       d_pl = dalloc(NS * cells, "d_planes"), fl = dalloc(F, "d_flags"), ce = dalloc((size_t)F * 4, "d_centres"),
       ro = dalloc((size_t)F * sizeof(mt_dir_rose), "d_rose"), fw = dalloc(flow_words * 4u, "d_flow");
  dbuf *all[8] = {&d_rec, &d_off, &d_so, &d_pl, &fl, &ce, &ro, &fw};
  HIP(hipMemcpy(d_rec.p, rec, sizeof rec, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_off.p, off, sizeof off, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_so.p, soff, sizeof soff, hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_pl.p, planes, NS * cells, hipMemcpyHostToDevice));

  /* ---- every refusal of the plane scan: the argument is named, no output byte changes, the canaries stand */
  unsigned char *host_out = malloc((size_t)F * sizeof(mt_dir_rose));
  if (!host_out) return 2;
  struct {
    const char *name, *word;
    int rec_bytes; const uint64_t *off, *so; uint32_t ns; const uint8_t *pl; uint8_t *fl; uint32_t *ce; mt_dir_rose *ro;
  } bad[] = {
      {"d_planes NULL", "d_planes", 8, (uint64_t *)d_off.p, (uint64_t *)d_so.p, NS, NULL, fl.p, (uint32_t *)ce.p, (mt_dir_rose *)ro.p},
      {"rec_bytes 16", "rec_bytes", 16, (uint64_t *)d_off.p, NULL, 0, d_pl.p, fl.p, (uint32_t *)ce.p, (mt_dir_rose *)ro.p},
      {"all outputs NULL", "all NULL", 8, (uint64_t *)d_off.p, NULL, 0, d_pl.p, NULL, NULL, NULL},
      {"d_frame_off NULL", "d_frame_off", 8, NULL, NULL, 0, d_pl.p, fl.p, (uint32_t *)ce.p, (mt_dir_rose *)ro.p},
      {"d_stream_off without n_streams", "n_streams", 8, (uint64_t *)d_off.p, (uint64_t *)d_so.p, 0, d_pl.p, fl.p, (uint32_t *)ce.p,
       (mt_dir_rose *)ro.p},
      {"n_streams without d_stream_off", "d_stream_off", 8, (uint64_t *)d_off.p, NULL, NS, d_pl.p, fl.p, (uint32_t *)ce.p,
       (mt_dir_rose *)ro.p},
      {"d_frame_off misaligned", "d_frame_off", 8, (uint64_t *)(d_off.p + 4), NULL, 0, d_pl.p, fl.p, (uint32_t *)ce.p, (mt_dir_rose *)ro.p},
      {"d_stream_off misaligned", "d_stream_off", 8, (uint64_t *)d_off.p, (uint64_t *)(d_so.p + 4), NS, d_pl.p, fl.p, (uint32_t *)ce.p,
       (mt_dir_rose *)ro.p},
      {"d_rose misaligned", "d_rose", 8, (uint64_t *)d_off.p, NULL, 0, d_pl.p, fl.p, (uint32_t *)ce.p, (mt_dir_rose *)(ro.p + 2)},
      {"d_centres misaligned", "d_centres", 8, (uint64_t *)d_off.p, NULL, 0, d_pl.p, fl.p, (uint32_t *)(ce.p + 1), (mt_dir_rose *)ro.p},
      {"d_rose in host memory", "d_rose is not memory of device", 8, (uint64_t *)d_off.p, NULL, 0, d_pl.p, fl.p, (uint32_t *)ce.p,
       (mt_dir_rose *)host_out},
      {"d_flags in host memory", "d_flags is not memory of device", 8, (uint64_t *)d_off.p, NULL, 0, d_pl.p, host_out, (uint32_t *)ce.p,
       (mt_dir_rose *)ro.p},
  };
  for (size_t i = 0; i < sizeof bad / sizeof bad[0]; ++i) {
    memset(host_out, FILL, (size_t)F * sizeof(mt_dir_rose));
    const int rc = mtgpu_scan_lanes_device(ctx, d_rec.p, bad[i].rec_bytes, (uint64_t)F * PER, bad[i].off, NULL, F, bad[i].so, bad[i].ns,
                                           bad[i].pl, bad[i].fl, bad[i].ce, bad[i].ro, NULL);
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
    for (int b = 0; b < 8; ++b) canary_check(all[b], bad[i].name);
  }
  /* ... and of the flow map */
  struct {
    const char *name, *word;
    int rec_bytes; const uint64_t *off, *so; uint32_t *flow;
  } badf[] = {
      {"d_flow NULL", "d_flow", 8, (uint64_t *)d_off.p, (uint64_t *)d_so.p, NULL},
      {"flow rec_bytes 12", "rec_bytes", 12, (uint64_t *)d_off.p, (uint64_t *)d_so.p, (uint32_t *)fw.p},
      {"flow d_stream_off NULL", "d_stream_off", 8, (uint64_t *)d_off.p, NULL, (uint32_t *)fw.p},
      {"flow d_frame_off NULL", "d_frame_off", 8, NULL, (uint64_t *)d_so.p, (uint32_t *)fw.p},
      {"d_flow misaligned", "d_flow", 8, (uint64_t *)d_off.p, (uint64_t *)d_so.p, (uint32_t *)(fw.p + 2)},
      {"d_flow in host memory", "d_flow is not memory of device", 8, (uint64_t *)d_off.p, (uint64_t *)d_so.p, (uint32_t *)host_out},
  };
  for (size_t i = 0; i < sizeof badf / sizeof badf[0]; ++i) {
    memset(host_out, FILL, (size_t)F * sizeof(mt_dir_rose));
    const int rc = mtgpu_flow_map_device(ctx, d_rec.p, badf[i].rec_bytes, (uint64_t)F * PER, badf[i].off, NULL, F, badf[i].so, NS,
                                         badf[i].flow, NULL);
    if (rc != MT_ERR_INVALID || !strstr(mtgpu_last_error(), badf[i].word)) {
      fprintf(stderr, "FAIL %s: rc %d, \"%s\" (want MT_ERR_INVALID naming \"%s\")\n", badf[i].name, rc, mtgpu_last_error(), badf[i].word);
      ++failures;
    }
    HIP(hipDeviceSynchronize());
    untouched(&fw, badf[i].name);
    for (size_t k = 0; k < (size_t)F * sizeof(mt_dir_rose); ++k)
      if (host_out[k] != FILL) {
        fprintf(stderr, "FAIL %s: the host buffer was written\n", badf[i].name);
        ++failures;
        break;
      }
    for (int b = 0; b < 8; ++b) canary_check(all[b], badf[i].name);
  }
  /* n_frames == 0 / n_streams == 0: MT_OK, and nothing is touched */
  MT(mtgpu_scan_lanes_device(ctx, NULL, 8, 0, NULL, NULL, 0, NULL, 0, d_pl.p, fl.p, (uint32_t *)ce.p, (mt_dir_rose *)ro.p, NULL));
  MT(mtgpu_flow_map_device(ctx, d_rec.p, 8, (uint64_t)F * PER, (uint64_t *)d_off.p, NULL, F, (uint64_t *)d_so.p, 0, (uint32_t *)fw.p, NULL));
  HIP(hipDeviceSynchronize());
  untouched(&fl, "n_frames 0");
  untouched(&ce, "n_frames 0");
  untouched(&ro, "n_frames 0");
  untouched(&fw, "n_streams 0");

  /* ---- the plane scan, every buffer at its stated size: all outputs, then each alone; with streams, then one plane */
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
        MT(mtgpu_scan_lanes_device(ctx, d_rec.p, 8, (uint64_t)F * PER, (uint64_t *)d_off.p, NULL, F, (uint64_t *)d_so.p, NS, d_pl.p, a, b, c,
                                   NULL));
      else      /* the last plane alone, W everywhere: it begins 2 * cells bytes into the buffer */
        MT(mtgpu_scan_lanes_device(ctx, d_rec.p, 8, (uint64_t)F * PER, (uint64_t *)d_off.p, NULL, F, NULL, 0, d_pl.p + 2 * cells, a, b, c,
                                   NULL));
      HIP(hipDeviceSynchronize());
      HIP(hipMemcpy(h_fl, fl.p, sizeof h_fl, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_ce, ce.p, sizeof h_ce, hipMemcpyDeviceToHost));
      HIP(hipMemcpy(h_ro, ro.p, sizeof h_ro, hipMemcpyDeviceToHost));
      for (uint32_t f = 0; f < F; ++f) {
        /* three cells in a row: 3 centres per allowed direction; a frame outside the streams reads 0 */
        const int live = form == 1 || (f >= soff[0] && f < soff[NS]);
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
      for (int k = 0; k < 8; ++k) canary_check(all[k], "mtgpu_scan_lanes_device");
    }

  /* ---- the flow map at its stated size: stream 0 owns 18 frames, stream 1 none, stream 2 sixteen */
  MT(mtgpu_flow_map_device(ctx, d_rec.p, 8, (uint64_t)F * PER, (uint64_t *)d_off.p, NULL, F, (uint64_t *)d_so.p, NS, (uint32_t *)fw.p, NULL));
  HIP(hipDeviceSynchronize());
  uint32_t *h_fw = malloc(flow_words * 4u);
  if (!h_fw) return 2;
  HIP(hipMemcpy(h_fw, fw.p, flow_words * 4u, hipMemcpyDeviceToHost));
  for (int s = 0; s < NS; ++s) {
    const uint32_t frames = (uint32_t)(soff[s + 1] - soff[s]);
    uint64_t total = 0;
    for (size_t i = 0; i < 8u * cells; ++i) total += h_fw[(size_t)s * 8u * cells + i];
    int ok = total == 6ull * frames;
    for (int x = 20; x < 23; ++x) {
      ok = ok && h_fw[(((size_t)s * 8u + 0u) * (size_t)p.grid_h + 10u) * (size_t)p.grid_w + (size_t)x] == frames;
      ok = ok && h_fw[(((size_t)s * 8u + 4u) * (size_t)p.grid_h + 20u) * (size_t)p.grid_w + (size_t)x] == frames;
    }
    if (!ok) {
      fprintf(stderr, "FAIL flow map: stream %d of %u frames holds %llu records\n", s, frames, (unsigned long long)total);
      ++failures;
    }
  }
  for (int k = 0; k < 8; ++k) canary_check(all[k], "mtgpu_flow_map_device");

  for (int k = 0; k < 8; ++k) HIP(hipFree(all[k]->p));
  free(h_fw);
  free(host_out);
  free(planes);
  mtgpu_destroy(ctx);
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  printf("all lanes buffers respected\n");
  return 0;
}
