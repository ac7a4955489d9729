// persist_kernels.hip — gfx950 kernels for temporal persistence (include/mtgpu_persist.h): per stream, the runs of motion
// frames — consecutive M frames that no break separates — and for every frame the length of its run and its place in it.
//
// One 256-lane workgroup per stream, as merge_streams_kernel launches.  The workgroup walks the stream in tiles of
// kPersistTile frames; a lane owns kPersistItems consecutive frames of a tile.  Everything is one segmented scan, used
// three times with different elements: a state is (mark, count), and
//     a . b = b.mark ? b : (a.mark, a.count + b.count)                                   (a before b in scan order)
// is associative with identity (0, 0).  A lane folds its own frames, the wave scans the lane totals with __shfl_up, the
// four wave totals meet in LDS behind ONE barrier, and the tile's total is carried into the next tile in registers.
//
//   forward walk, scan 1   M frame i: (i + 1, 0), Q: (0, 1), T: (0, 0).  The exclusive prefix of an M frame is
//                          (p + 1 or 0, q): its previous M frame and the Q frames between.  With the boxes of p and the
//                          frame itself that decides brk.
//   forward walk, scan 2   M frame: (brk, 1), else (0, 0).  The inclusive count of an M frame is pos.  pos goes to d_pos,
//                          or to d_work when d_pos is NULL.
//   backward walk          the tiles in descending order, a tile's frames in descending order.  M frame with pos == 1
//                          (a break): (1, 0), another M frame: (0, 1), else (0, 0).  The exclusive count of an M frame
//                          is the number of M frames behind it up to the next break: run = pos + that.
//
// No global atomics, no scratch ring, no allocation.  Every barrier sits in control flow that depends on the stream's
// bounds alone, which the whole workgroup reads alike.  stream_off entries are clamped to n_frames before anything is
// addressed, so offsets that lie (the device entry point trusts them) cannot reach outside the caller's arrays.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "persist_kernels.h"

#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "persist_kernels.hip is written for gfx950 only (wave64)"
#endif

namespace mtgpu {

namespace {

constexpr int PB = kPersistBlock;
constexpr int PK = kPersistItems;
constexpr int PT = kPersistTile;
constexpr int PW = PB / 64;
static_assert(PB % 64 == 0 && PT % PB == 0, "whole waves, whole lanes per tile");

struct St { unsigned int mark, count; };

__device__ __forceinline__ St comb(St a, St b) {
  St r;
  r.mark = b.mark ? b.mark : a.mark;
  r.count = b.mark ? b.count : a.count + b.count;
  return r;
}

// x[0 .. PK) are the lane's elements in scan order (lane l owns scan positions l * PK ..).  On return x[j] is the
// inclusive prefix of position j and *before the prefix in front of x[0], both with `carry` (everything scanned in
// earlier tiles) in front; carry becomes the prefix behind the tile.  ws: PW states in LDS that no lane still reads
// from an earlier call — the callers alternate between two buffers, which one barrier per call keeps apart.
__device__ __forceinline__ void tile_scan(St (&x)[PK], St &carry, St *ws, St *before) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 1; j < PK; ++j) x[j] = comb(x[j - 1], x[j]);
  St t = x[PK - 1];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    St o;
    o.mark = __shfl_up(t.mark, d);
    o.count = __shfl_up(t.count, d);
    if (lane >= d) t = comb(o, t);
  }
  St e;
  e.mark = __shfl_up(t.mark, 1);
  e.count = __shfl_up(t.count, 1);
  if (lane == 0) e.mark = e.count = 0u;
  if (lane == 63) ws[wave] = t;
  __syncthreads();
  St pre = carry, tot = carry;
#pragma unroll
  for (int w = 0; w < PW; ++w) {
    const St s = ws[w];
    tot = comb(tot, s);
    if (w < wave) pre = comb(pre, s);
  }
  carry = tot;
  pre = comb(pre, e);
  *before = pre;
#pragma unroll
  for (int j = 0; j < PK; ++j) x[j] = comb(pre, x[j]);
}

// include/mtgpu_persist.h: linked(A, B); 32-bit arithmetic, reach <= 65535
__device__ __forceinline__ bool linked(PersistBox a, PersistBox b, unsigned int reach) {
  const bool none_a = (a.x0 & a.y0 & a.x1 & a.y1) == 0xFFFFu, none_b = (b.x0 & b.y0 & b.x1 & b.y1) == 0xFFFFu;
  if (none_a || none_b) return false;
  return (unsigned int)b.x0 <= (unsigned int)a.x1 + reach && (unsigned int)a.x0 <= (unsigned int)b.x1 + reach &&
         (unsigned int)b.y0 <= (unsigned int)a.y1 + reach && (unsigned int)a.y0 <= (unsigned int)b.y1 + reach;
}

}  // namespace

// Frames outside [stream_off[0], stream_off[n_streams]) read 0 in every non-null output.
__global__ __launch_bounds__(PB) void persist_clear_kernel(const unsigned long long *__restrict__ stream_off, unsigned int n_streams,
                                                           unsigned int n_frames, unsigned char *__restrict__ flags_out,
                                                           unsigned int *__restrict__ run, unsigned int *__restrict__ pos) {
  unsigned long long lo = stream_off[0], hi = stream_off[n_streams];
  if (lo > n_frames) lo = n_frames;
  if (hi > n_frames) hi = n_frames;
  if (hi < lo) hi = lo;
  const unsigned long long step = (unsigned long long)gridDim.x * PB;
  for (unsigned long long f = (unsigned long long)blockIdx.x * PB + threadIdx.x; f < n_frames; f += step) {
    if (f >= lo && f < hi) continue;
    if (flags_out) flags_out[f] = 0;
    if (run) run[f] = 0u;
    if (pos) pos[f] = 0u;
  }
}

__global__ __launch_bounds__(PB) void persist_streams_kernel(
    const unsigned char *__restrict__ flags, const unsigned char *__restrict__ has_sd, const PersistBox *__restrict__ box,
    unsigned int n_frames, const unsigned long long *__restrict__ stream_off, unsigned int n_streams, unsigned int need,
    unsigned int max_dropout, unsigned int reach, unsigned int *__restrict__ work, unsigned char *__restrict__ flags_out,
    unsigned int *__restrict__ run, unsigned int *__restrict__ pos) {
  __shared__ St ws[2][PW];
  unsigned int *const posbuf = pos ? pos : work;
  const unsigned int first = threadIdx.x * PK;           // the lane's first scan position in a tile

  for (unsigned int s = blockIdx.x; s < n_streams; s += gridDim.x) {
    unsigned long long b = stream_off[s], e = stream_off[s + 1];
    if (b > n_frames) b = n_frames;
    if (e > n_frames) e = n_frames;
    if (e < b) e = b;
    const unsigned long long len = e - b;                // < 2^32
    const unsigned long long tiles = (len + PT - 1) / PT;

    // ---- forward: previous M frame and the Q frames since, brk, pos
    St carry_a = {0u, 0u}, carry_b = {0u, 0u};
    for (unsigned long long t = 0; t < tiles; ++t) {
      const unsigned long long i0 = t * PT + first;      // the lane's first frame, relative to the stream
      bool is_m[PK];
      St x[PK];
#pragma unroll
      for (int j = 0; j < PK; ++j) {
        const unsigned long long i = i0 + j;
        is_m[j] = false;
        x[j].mark = x[j].count = 0u;
        if (i < len) {
          if (flags[b + i] != 0) {
            is_m[j] = true;
            x[j].mark = (unsigned int)i + 1u;
          } else if (!has_sd || has_sd[b + i] != 0) {
            x[j].count = 1u;                              // Q; a T frame stays (0, 0)
          }
        }
      }
      St before;
      tile_scan(x, carry_a, ws[0], &before);
      St y[PK];
#pragma unroll
      for (int j = 0; j < PK; ++j) {
        y[j].mark = y[j].count = 0u;
        if (is_m[j]) {
          const St prev = j ? x[j - 1] : before;          // (p + 1 or 0, Q frames since p)
          bool brk = prev.mark == 0u || prev.count > max_dropout;
          if (!brk && box) brk = !linked(box[b + (prev.mark - 1u)], box[b + i0 + j], reach);
          y[j].mark = brk ? 1u : 0u;
          y[j].count = 1u;
        }
      }
      tile_scan(y, carry_b, ws[1], &before);
#pragma unroll
      for (int j = 0; j < PK; ++j)
        if (i0 + j < len) posbuf[b + i0 + j] = is_m[j] ? y[j].count : 0u;
    }

    __syncthreads();                                      // pos is read back by other lanes than wrote it

    // ---- backward: the M frames behind a frame up to the next break; run, flags_out
    St carry_c = {0u, 0u};
    for (unsigned long long t = tiles; t-- > 0;) {
      const unsigned long long top = t * PT + (PT - 1);   // scan position 0 is the tile's last frame
      unsigned int p[PK];
      St x[PK];
#pragma unroll
      for (int j = 0; j < PK; ++j) {
        const unsigned long long i = top - (first + j);
        p[j] = i < len ? posbuf[b + i] : 0u;
        x[j].mark = p[j] == 1u ? 1u : 0u;
        x[j].count = p[j] > 1u ? 1u : 0u;
      }
      St before;
      tile_scan(x, carry_c, ws[t & 1], &before);
#pragma unroll
      for (int j = 0; j < PK; ++j) {
        const unsigned long long i = top - (first + j);
        if (i < len) {
          const St behind = j ? x[j - 1] : before;
          const unsigned int r = p[j] ? p[j] + behind.count : 0u;
          if (run) run[b + i] = r;
          if (flags_out) flags_out[b + i] = r >= need ? 1 : 0;
        }
      }
    }
    __syncthreads();                                      // the next stream's first scan reuses ws[0]
  }
}

hipError_t launch_persist(const PersistLaunch &L) {
  if (L.n_frames == 0 || L.n_streams == 0) return hipSuccess;
  if (!L.flags || !L.stream_off || !L.work || L.need == 0u || (!L.flags_out && !L.run && !L.pos)) return hipErrorInvalidValue;
  const unsigned long long clear_blocks = ((unsigned long long)L.n_frames + PB - 1u) / PB;
  hipLaunchKernelGGL(persist_clear_kernel, dim3(clear_blocks < 1024u ? (unsigned int)clear_blocks : 1024u), dim3(PB), 0, L.stream, L.stream_off,
                     L.n_streams, L.n_frames, L.flags_out, L.run, L.pos);
  hipLaunchKernelGGL(persist_streams_kernel, dim3(L.n_streams < 65536u ? L.n_streams : 65536u), dim3(PB), 0, L.stream, L.flags,
                     L.has_sd, L.box, L.n_frames, L.stream_off, L.n_streams, L.need, L.max_dropout, L.reach, L.work, L.flags_out,
                     L.run, L.pos);
  return hipGetLastError();
}

}  // namespace mtgpu
