// scalar_kernels.hip — the reference's per-second "motion scalar" (tools/motion_scalar.cpp:61-84, BASELINE config 1)
// on gfx950, over the same 40-byte AVMotionVector records the scan streams.
//
//   motion_scores_kernel   one workgroup per entry of the scan's work list (plan_frames: frames with records, in stream
//                          order; frames without never cost a workgroup): the frame's
//                              sum over records with motion_scale != 0 of  sqrt(dx^2 + dy^2) * w * h      (:75-82)
//                          and the number of those records.
//   motion_bins_kernel     per stream: acc[floor(pts)] += the frame's score, frames in ascending order  (:62-66, :82).
//
// Arithmetic.  A term is computed in fp64 in the reference's order — dx = double(mx) / scale, dy = double(my) / scale,
// mag = sqrt(dx * dx + dy * dy), term = (mag * w) * h — with IEEE division and square root and no contraction
// (-ffp-contract=off, csrc/Makefile): every term has the bits the CPU computes.  When every motion_scale of a wave
// instruction is a power of two (FFmpeg exports 4) the two divisions become multiplications by the exact reciprocal
// 2^-k, which round identically (the quotient of an int32 by 2^k, k <= 15, is exact either way).
// Summation.  A frame's sum follows a fixed tree: every lane adds its own records in stream order, the 64 lanes of a
// wave are combined by a butterfly (xor 32, 16, .. 1), the wave totals go through LDS and are added in wave order by
// lane 0, which stores the result.  No floating-point atomics, nothing depends on arrival order: the same call on the
// same buffers returns the same bits.  (Which lane a record goes to depends on the address of the frame's first record
// modulo 128 — the head peel below — so the SAME records at another address may round differently in the last place.)
#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "scalar_kernels.hip is written for gfx950 only (wave64, sc1 write-through stores)"
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scalar_kernels.h"
#include "record_stream.h"

namespace mtgpu {

namespace {

// What a term needs of a record (layout: include/mt_types.h, mt_mv): bytes 4-5 (w, h; the dword at +4 also carries
// src_x) and bytes 24-33 (motion_x, motion_y, motion_scale; the three dwords at +24 also carry two padding bytes).
// Both with the streaming (nt) hint: every record is read once.
struct RecFields {
  unsigned int wh;
  u32x3 m;
};
__device__ __forceinline__ RecFields load_rec(const unsigned char *rec) {
  RecFields r;
  r.wh = __builtin_nontemporal_load(reinterpret_cast<const unsigned int *>(rec + 4));
  r.m = __builtin_nontemporal_load(reinterpret_cast<const u32x3_a4 *>(rec + 24));
  return r;
}

__device__ __forceinline__ unsigned int scale_of(const RecFields &r) { return r.m.z & 0xffffu; }
// motion_scale is zero (the record is skipped, :75-76) or a power of two
__device__ __forceinline__ bool scale_is_pow2(unsigned int s) { return (s & (s - 1u)) == 0u; }

// One record's term (:75-82) added to the lane's partial sum.  POW2 (wave-uniform): every scale of this wave
// instruction is a power of two.
template <bool POW2>
__device__ __forceinline__ void add_term(const RecFields &r, double &acc, unsigned int &cnt) {
  const unsigned int scale = scale_of(r);
  if (scale == 0u) return;                                             // :75-76
  const double mx = (double)(int)r.m.x, my = (double)(int)r.m.y;
  double dx, dy;
  if constexpr (POW2) {
    // 2^-k exactly, k = log2(scale) <= 15
    const double rcp = __longlong_as_double((long long)(1023u - (unsigned int)__builtin_ctz(scale)) << 52);
    dx = mx * rcp;
    dy = my * rcp;
  } else {
    const double s = (double)(int)scale;
    dx = mx / s;                                                       // :78-79
    dy = my / s;
  }
  const double mag = sqrt(dx * dx + dy * dy);                          // :81
  const double w = (double)(int)(r.wh & 0xffu), h = (double)(int)((r.wh >> 8) & 0xffu);
  acc += (mag * w) * h;                                                // :82
  ++cnt;
}

// `ok`: this lane holds a record.  The choice of the path is made per wave instruction, in uniform control flow.
__device__ __forceinline__ void add_term_any(const RecFields &r, bool ok, double &acc, unsigned int &cnt) {
  const bool pow2 = __all(!ok || scale_is_pow2(scale_of(r))) != 0;
  if (pow2) { if (ok) add_term<true>(r, acc, cnt); }
  else { if (ok) add_term<false>(r, acc, cnt); }
}

}  // namespace

// scores[f] = +0.0, terms[f] = 0 for every frame, ahead of the scores kernel on the same stream: the planner lists
// only frames with records, the others keep these values.
__global__ __launch_bounds__(256) void motion_clear_kernel(double *__restrict__ scores, unsigned int *__restrict__ terms,
                                                           unsigned int n_frames, int sys_scores, int sys_terms) {
  for (unsigned long long f = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; f < n_frames;
       f += (unsigned long long)gridDim.x * 256ull) {
    store_result(&scores[f], 0.0, sys_scores);
    if (terms) store_result(&terms[f], 0u, sys_terms);
  }
}

template <int BLOCK, int UNROLL>
__global__ __launch_bounds__(BLOCK) void motion_scores_kernel(
    const unsigned char *__restrict__ mv, const WorkItem *__restrict__ work, unsigned int item0, unsigned int n_items,
    double *__restrict__ scores, unsigned int *__restrict__ terms, int sys_scores, int sys_terms) {
  constexpr int WAVES = BLOCK / 64;
  __shared__ double wave_sum[WAVES];
  __shared__ unsigned int wave_cnt[WAVES];
  const unsigned int item = item0 + blockIdx.x;
  if (item >= n_items) return;
  const WorkItem me = load_item(work, item);
  if (me.f == kNoFrame) return;                 // the list has ended (every later entry is past its end too)
  const int tid = threadIdx.x;
  const unsigned char *base = mv + me.r0 * 40ull;
  unsigned long long n = me.r1 - me.r0;
  double acc = 0.0;
  unsigned int cnt = 0u;
  // The streaming loop is this kernel's own, not record_stream.h's: it reads other fields of a record, chooses its
  // arithmetic per wave instruction with __all — so every lane of a wave must make every trip — and its summation
  // order is part of the result.
  // Head peel, as the scan's stream_mv40: a wave instruction of the loop below covers 64 records = 2560 bytes =
  // exactly 20 128-byte lines if the stream starts on a line.  40 h = -start (mod 128) has a solution h < 16 whenever
  // the start is 8-byte aligned (5 * 13 = 1 mod 16): the first h records go to lanes 0..h-1.
  const unsigned int r = (unsigned int)((uintptr_t)base & 127u);
  if ((r & 7u) == 0u) {
    unsigned long long h = (unsigned long long)((13u * ((16u - (r >> 3)) & 15u)) & 15u);
    h = h < n ? h : n;
    if (h != 0ull && tid < 64) {                // (wave 0 only, uniform per wave)
      const bool ok = (unsigned long long)tid < h;
      RecFields d = {0u, {0u, 0u, 0u}};
      if (ok) d = load_rec(base + (unsigned long long)tid * 40ull);
      add_term_any(d, ok, acc, cnt);
    }
    base += h * 40ull;
    n -= h;
  }
  unsigned long long i = tid;
  constexpr unsigned long long STEP = (unsigned long long)UNROLL * BLOCK;
  constexpr unsigned long long LAST = (unsigned long long)(UNROLL - 1) * BLOCK;
  for (; i + LAST < n; i += STEP) {             // lane i of a step takes record i, UNROLL x 2 independent loads in flight
    RecFields d[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) d[u] = load_rec(base + (i + (unsigned long long)u * BLOCK) * 40ull);
    bool p2 = true;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) p2 = p2 && scale_is_pow2(scale_of(d[u]));
    if (__all(p2)) {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) add_term<true>(d[u], acc, cnt);
    } else {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) add_term<false>(d[u], acc, cnt);
    }
  }
  // the rest (fewer than one step; `i - tid` is uniform, so every wave makes the same trips)
  if (i - (unsigned long long)tid < n) {
    RecFields d[UNROLL];
    bool ok[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const unsigned long long q = i + (unsigned long long)u * BLOCK;
      ok[u] = q < n;
      d[u] = RecFields{0u, {0u, 0u, 0u}};
      if (ok[u]) d[u] = load_rec(base + q * 40ull);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) add_term_any(d[u], ok[u], acc, cnt);
  }
  // the fixed tree: butterfly inside the wave, wave totals in wave order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o);
    cnt += (unsigned int)__shfl_xor((int)cnt, o);
  }
  if ((tid & 63) == 0) { wave_sum[tid >> 6] = acc; wave_cnt[tid >> 6] = cnt; }
  __syncthreads();
  if (tid == 0) {
    double s = wave_sum[0];
    unsigned int c = wave_cnt[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) { s += wave_sum[w]; c += wave_cnt[w]; }
    store_result(&scores[me.f], s, sys_scores);
    if (terms) store_result(&terms[me.f], c, sys_terms);
  }
}

// One workgroup per (stream, kBinsBlock bins): lane t owns bin blockIdx's first bin + t and walks the stream's frames
// in order, kBinsBlock at a time through LDS — a bin's frames are added in ascending frame order starting from +0.0,
// whatever the grid looks like.  A chunk none of whose frames falls into the workgroup's bins is skipped.
__global__ __launch_bounds__(kBinsBlock) void motion_bins_kernel(
    const double *__restrict__ scores, const unsigned int *__restrict__ terms, const double *__restrict__ pts,
    const unsigned long long *__restrict__ stream_off, unsigned int n_sec, unsigned int blocks_per_stream,
    double *__restrict__ acc, unsigned long long *__restrict__ bin_terms, int sys_acc, int sys_bin_terms) {
  __shared__ unsigned int c_sec[kBinsBlock];
  __shared__ unsigned int c_terms[kBinsBlock];
  __shared__ double c_score[kBinsBlock];
  const unsigned int s = blockIdx.x / blocks_per_stream, tid = threadIdx.x;
  const unsigned int bin0 = (blockIdx.x % blocks_per_stream) * (unsigned int)kBinsBlock;
  const unsigned int bin = bin0 + tid;
  const unsigned long long f0 = stream_off[s], f1 = stream_off[s + 1];
  double a = 0.0;
  unsigned long long t = 0ull;
  for (unsigned long long c0 = f0; c0 < f1; c0 += (unsigned long long)kBinsBlock) {
    const unsigned long long f = c0 + tid;
    unsigned int sec = 0xffffffffu;                       // skipped: null / negative (:62-63), NaN, past n_sec
    double sc = 0.0;
    unsigned int tm = 0u;
    if (f < f1) {
      const double p = pts[f];
      if (p >= 0.0) {
        const double fl = floor(p);                        // :66
        if (fl < (double)n_sec) { sec = (unsigned int)fl; sc = scores[f]; tm = terms ? terms[f] : 0u; }
      }
    }
    const bool mine = sec != 0xffffffffu && sec - bin0 < (unsigned int)kBinsBlock;   // (sec >= bin0, unsigned wrap otherwise)
    if (!__syncthreads_or(mine ? 1 : 0)) continue;         // (also orders the previous chunk's reads before the writes below)
    c_sec[tid] = sec; c_score[tid] = sc; c_terms[tid] = tm;
    __syncthreads();
    const unsigned int m = (unsigned int)(f1 - c0 < (unsigned long long)kBinsBlock ? f1 - c0 : (unsigned long long)kBinsBlock);
    for (unsigned int j = 0; j < m; ++j)
      if (c_sec[j] == bin) { a += c_score[j]; t += c_terms[j]; }
  }
  if (bin < n_sec) {
    const unsigned long long at = (unsigned long long)s * n_sec + bin;
    store_result(&acc[at], a, sys_acc);
    if (bin_terms) store_result(&bin_terms[at], t, sys_bin_terms);
  }
}

hipError_t launch_motion_scores(const ScoresLaunch &L) {
  if (L.n_frames == 0) return hipSuccess;
  if (!L.scores || !L.frame_off || !L.plan_ws || ((uintptr_t)L.plan_ws & 31u) != 0u || L.rebase > L.n_records)
    return hipErrorInvalidValue;
  {
    const unsigned int blocks = (L.n_frames + 255u) / 256u;
    hipLaunchKernelGGL(motion_clear_kernel, dim3(blocks < 1024u ? blocks : 1024u), dim3(256), 0, L.stream, L.scores,
                       L.terms, L.n_frames, L.sys_scores, L.sys_terms);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  // has_sd == null: a frame is listed iff it has records; flags / centres null: the planner answers nothing itself
  hipError_t e = plan_work_list(L.frame_off, nullptr, L.n_records, L.rebase, L.n_frames, L.plan_ws, L.stream, nullptr, nullptr, 0,
                                nullptr, 0);
  if (e != hipSuccess) return e;
  const WorkItem *work = static_cast<const WorkItem *>(L.plan_ws);
  return launch_chunked(L.n_frames, kGridChunk, [&](unsigned long long i0, unsigned int n) {
    hipLaunchKernelGGL((motion_scores_kernel<kScoresBlock, kScoresUnroll>), dim3(n), dim3(kScoresBlock), 0, L.stream, L.mv, work,
                       (unsigned int)i0, L.n_frames, L.scores, L.terms, L.sys_scores, L.sys_terms);
  });
}

hipError_t launch_motion_bins(const BinsLaunch &L) {
  if (L.n_streams == 0) return hipSuccess;
  if (L.n_sec == 0 || !L.scores || !L.pts || !L.stream_off || !L.acc || (L.bin_terms && !L.terms)) return hipErrorInvalidValue;
  const unsigned int per = (L.n_sec + (unsigned int)kBinsBlock - 1u) / (unsigned int)kBinsBlock;
  const unsigned long long blocks = (unsigned long long)per * L.n_streams;
  if (blocks >= (1ull << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(motion_bins_kernel, dim3((unsigned int)blocks), dim3(kBinsBlock), 0, L.stream, L.scores, L.terms, L.pts,
                     L.stream_off, L.n_sec, per, L.acc, L.bin_terms, L.sys_acc, L.sys_bin_terms);
  return hipGetLastError();
}

}  // namespace mtgpu
