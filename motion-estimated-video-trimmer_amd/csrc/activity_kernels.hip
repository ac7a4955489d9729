// activity_kernels.hip — per-stream activity maps: for every grid cell, the number of frames of a stream in which
// the cell was active (votes >= vectors_needed, src/motion_scanner.cpp:242-268, :282) and the number in which it was
// one of the centres :277-292 counts (without the early return).  The first output of the library that accumulates
// ACROSS frames.
//
//   activity_clear_kernel    zero-fills one output ahead of the map kernel: the call clears, then counts.
//   activity_frames_kernel   one workgroup per RUN of k.run consecutive entries of the scan's work list (plan_frames:
//                            the frames with side data, in stream order).  Surplus workgroups find kNoFrame and leave.
//     per frame   zero the vote tile; stream the records as the sweep does with one threshold (head peel to a 128-byte
//                 line, non-temporal loads, kActUnroll in flight per lane, one fire-and-forget `ds_add_u32` per kept
//                 record); the 64-bit masks of the active cells of every tracked row and of the centres of every
//                 analysed row, and the frame's centre count; then ONE uniform branch: does the frame contribute
//                 (count >= min_centres)?
//     ACC > 0     a contributing frame adds its two masks into two planes of LDS accumulators, one field per cell.
//                 Every lane owns fixed groups of four cells: a plain LDS read-modify-write, no atomics.
//     flush       when the run ends, when max_run frames have been collected (a 16-bit field never wraps) and when the
//                 next entry belongs to another stream: every non-zero field is added to the stream's map with a
//                 no-return `global_atomic_add_u32` (agent scope, relaxed), lane i of a wave-instruction on cell i of
//                 64 consecutive cells — the analysed rows of a plane are one contiguous block, so each instruction
//                 covers one contiguous 256-byte segment — and the field is zeroed; one atomic for d_frames[s].
//     ACC == 0    no room for accumulators next to the tile (4K at small margins): a contributing frame adds its masks
//                 to the map directly, one atomic per set bit.
//   Integer adds commute: the maps are bit-reproducible whatever the run length, the launch grid or the order in which
//   workgroups arrive.  That is why this is integer atomics and not a slab reducer: nothing has to be ordered.
//
// The record loads, the streamers, the vote, the row masks and the centre test of a word are those of record_stream.h,
// shared with sweep_kernels.hip and zones_kernels.hip and instantiated here with this kernel's functors; the launch
// helpers are those of scan_kernels.h.  A change there must leave this file's device assembly as it was.
#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "activity_kernels.hip is written for gfx950 only (wave64, 160 KB LDS)"
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "activity_kernels.h"
#include "record_stream.h"

namespace mtgpu {

namespace {

// ---- the centres (:277-293), one task per (analysed row, word): analysed row r <-> mask row r + 1; x in [1, gw-2]
// (:280); neighbours across word and row boundaries; outside the grid: inactive.  The sweep's count_centres, which
// also keeps the mask of the centres it counts.
template <int BLOCK>
__device__ __forceinline__ void centre_masks(const unsigned long long *amask, unsigned long long *cmask, unsigned int *total,
                                             const ActK &k, int crows) {
  const int W = k.W;
  const int ntask = crows * W;
  for (int tk = threadIdx.x; tk < ntask; tk += BLOCK) {
    const int r = tk / W, w = tk - r * W;
    const unsigned long long cm = centre_word(amask + (size_t)(r + 1) * W, w, W, k.gw);
    cmask[tk] = cm;
    const unsigned int c = (unsigned int)__popcll(cm);
    if (c) atomicAdd(total, c);
  }
}

// No-return vector atomic on global memory: agent scope (adders sit on all eight XCDs), relaxed — only the sum matters.
__device__ __forceinline__ void global_add(unsigned int *p, unsigned int v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Four mask bits into four accumulator fields.
__device__ __forceinline__ unsigned long long spread16(unsigned int b) {
  return (unsigned long long)(b & 1u) | ((unsigned long long)(b & 2u) << 15) | ((unsigned long long)(b & 4u) << 30) |
         ((unsigned long long)(b & 8u) << 45);
}

// A contributing frame's masks into the accumulators.  Unit u = fields 4u .. 4u + 3 of a plane of crows x gwp fields,
// always the same lane's: analysed row r = u / (gwp / 4), cells x0 .. x0 + 3, x0 = 4 (u % (gwp / 4)) — four bits of one
// mask word (x0 is a multiple of 4).  Bits of cells outside the grid are 0 in both masks.
template <int BLOCK, int ACC>
__device__ __forceinline__ void accumulate(const unsigned long long *amask, const unsigned long long *cmask, unsigned char *acc_a,
                                           unsigned char *acc_c, const ActK &k, int crows) {
  const int upr = k.gwp >> 2, units = crows * upr;
  for (int u = threadIdx.x; u < units; u += BLOCK) {
    const int r = u / upr, x0 = (u - r * upr) << 2;
    const unsigned int ba = (unsigned int)(amask[(size_t)(r + 1) * k.W + (x0 >> 6)] >> (x0 & 63)) & 15u;
    if (ba == 0u) continue;                                    // a centre is an active cell
    const unsigned int bc = (unsigned int)(cmask[(size_t)r * k.W + (x0 >> 6)] >> (x0 & 63)) & 15u;
    if constexpr (ACC == 16) {
      reinterpret_cast<unsigned long long *>(acc_a)[u] += spread16(ba);
      if (bc) reinterpret_cast<unsigned long long *>(acc_c)[u] += spread16(bc);
    } else {
      reinterpret_cast<u32x4 *>(acc_a)[u] += (u32x4){ba & 1u, (ba >> 1) & 1u, (ba >> 2) & 1u, ba >> 3};
      if (bc) reinterpret_cast<u32x4 *>(acc_c)[u] += (u32x4){bc & 1u, (bc >> 1) & 1u, (bc >> 2) & 1u, bc >> 3};
    }
  }
}

// One accumulator plane into one plane of stream s's map, and zeroed.  Cell c = r * gw + x of the analysed rows is
// word y_lo * gw + c of the plane: lane i of a wave takes cell i of 64 consecutive cells, so one wave-instruction of
// atomics covers one contiguous 256-byte segment.  Integer adds commute: no order is needed for reproducible maps.
template <int BLOCK, int ACC>
__device__ __forceinline__ void flush_plane(unsigned char *acc, unsigned int *__restrict__ out, const ActK &k, int crows) {
  const int cells = crows * k.gw;
  for (int c = threadIdx.x; c < cells; c += BLOCK) {
    const int r = c / k.gw, x = c - r * k.gw;
    const size_t at = (size_t)r * k.gwp + x;
    unsigned int v;
    if constexpr (ACC == 16) v = reinterpret_cast<unsigned short *>(acc)[at];
    else v = reinterpret_cast<unsigned int *>(acc)[at];
    if (v == 0u) continue;
    if (out) global_add(out + c, v);
    if constexpr (ACC == 16) reinterpret_cast<unsigned short *>(acc)[at] = (unsigned short)0;
    else reinterpret_cast<unsigned int *>(acc)[at] = 0u;
  }
}

// ACC == 0: one frame's mask plane straight into the map, one atomic per set bit.  first_row: the mask row of analysed
// row 0 (1 for the active masks, 0 for the centre masks).
template <int BLOCK>
__device__ __forceinline__ void flush_mask(const unsigned long long *mask, int first_row, unsigned int *__restrict__ out,
                                           const ActK &k, int crows) {
  const int cells = crows * k.gw;
  for (int c = threadIdx.x; c < cells; c += BLOCK) {
    const int r = c / k.gw, x = c - r * k.gw;
    if ((mask[(size_t)(r + first_row) * k.W + (x >> 6)] >> (x & 63)) & 1ull) global_add(out + c, 1u);
  }
}

}  // namespace

__global__ __launch_bounds__(256) void activity_clear_kernel(unsigned int *__restrict__ out, unsigned long long n) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull)
    out[i] = 0u;
}

// Waves per SIMD: a workgroup is 16 waves, four per SIMD.  The forms with accumulators are planned for two resident
// workgroups per CU (mtgpu_api.hip, activity_plan), which takes eight waves per SIMD and so at most 64 VGPRs; left alone
// the register allocator takes 76-79 and one workgroup would sit alone on its CU, idle at every barrier.  The form
// without accumulators (4K) fills LDS with one workgroup and keeps its registers.
template <int BLOCK, int UNROLL, int REC, int ACC>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(ACC != 0 ? 8 : 4, 8))) void activity_frames_kernel(
    const unsigned char *__restrict__ mv, const WorkItem *__restrict__ work, unsigned int wg0, unsigned int n_frames, ActK k,
    const unsigned long long *__restrict__ stream_off, unsigned int n_streams, unsigned int *__restrict__ active,
    unsigned int *__restrict__ centre, unsigned int *__restrict__ frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned int lds[];
  const unsigned long long first = ((unsigned long long)wg0 + blockIdx.x) * (unsigned long long)k.run;
  if (first >= n_frames) return;
  WorkItem it = load_item(work, first);
  if (it.f == kNoFrame) return;                 // the list has ended (every later entry is past its end too)
  const int tid = threadIdx.x;
  const size_t plane = ACC ? (size_t)k.R * k.gwp * (ACC / 8) : 0u;
  unsigned int *tile = lds;
  unsigned char *acc_a = reinterpret_cast<unsigned char *>(lds + k.tile_words);
  unsigned char *acc_c = acc_a + plane;
  unsigned long long *amask = reinterpret_cast<unsigned long long *>(acc_c + plane);
  unsigned long long *cmask = amask + (size_t)(k.R + 2) * k.W;
  unsigned int *total = reinterpret_cast<unsigned int *>(cmask + (size_t)k.R * k.W);
  const int t0 = max(k.y_lo - 1, 0), t1 = min(k.y_hi + 1, k.gh);
  const int crows = k.y_hi - k.y_lo;
  const size_t plane_words = (size_t)k.gh * k.gw, rows_at = (size_t)k.y_lo * k.gw;

  if constexpr (ACC != 0) {                     // both planes (the first accumulation is several barriers away)
    unsigned long long *a8 = reinterpret_cast<unsigned long long *>(acc_a);
    const int n8 = (int)((2u * plane) >> 3);
    for (int i = tid; i < n8; i += BLOCK) a8[i] = 0ull;
  }

  // The run's first stream, where the forward walk below starts: s = the number of streams that end at or before frame f.
  // s == n_streams: the frame lies behind the last stream and is counted nowhere.  record_stream.h's stream_of written
  // out: with the call the 4K form measured 1 % slower (docs/rounds/r24_kernel_fold.md).
  unsigned int s = 0u;
  {
    unsigned int lo = 0u, hi = n_streams;
    const unsigned int f = __builtin_amdgcn_readfirstlane(it.f);
    while (lo < hi) {
      const unsigned int mid = lo + ((hi - lo) >> 1);
      if (stream_off[mid + 1u] <= (unsigned long long)f) lo = mid + 1u; else hi = mid;
    }
    s = lo;
  }
  unsigned int pend = 0u;                       // contributing frames in the accumulators (ACC == 0: always 0)

  const auto flush = [&]() {                    // workgroup-uniform: s < n_streams, pend > 0
    __syncthreads();                            // accumulated by unit, flushed by cell
    flush_plane<BLOCK, ACC>(acc_a, active ? active + (size_t)s * plane_words + rows_at : nullptr, k, crows);
    flush_plane<BLOCK, ACC>(acc_c, centre ? centre + (size_t)s * plane_words + rows_at : nullptr, k, crows);
    if (frames && tid == 0) global_add(frames + s, pend);
    pend = 0u;
  };

  for (int i = 0; i < k.run; ++i) {
    if (i > 0) {
      if (first + (unsigned long long)i >= n_frames) break;
      it = load_item(work, first + (unsigned long long)i);
      if (it.f == kNoFrame) break;
    }
    const unsigned int f = __builtin_amdgcn_readfirstlane(it.f);
    if (s < n_streams && stream_off[s + 1u] <= (unsigned long long)f) {       // the entry belongs to another stream
      if constexpr (ACC != 0) { if (pend) flush(); }
      do ++s; while (s < n_streams && stream_off[s + 1u] <= (unsigned long long)f);
    }
    if (s >= n_streams) break;

    // ---- zero the tile (record_stream.h's zero_tile written out: the call moves the register counts of the ACC 0 forms).
    // The compact forms with accumulators make the zeros per frame: held across the run loop they take the four VGPRs
    // those forms lack under 64, and two lane offsets of the streamer went to scratch (docs/rounds/r24_kernel_fold.md).
    {
      u32x4 *c4 = reinterpret_cast<u32x4 *>(tile);
      const int n4 = k.tile_words >> 2;
      u32x4 zero = (u32x4){0u, 0u, 0u, 0u};
      if constexpr (ACC != 0 && REC == 8) asm volatile("" : "+v"(zero));
      for (int j = tid; j < n4; j += BLOCK) c4[j] = zero;
    }
    __syncthreads();
    // ---- the votes (an empty analysed range keeps nothing: nothing to read)
    if (crows > 0) {
      const auto one = [=, &k](const MvFields m) { vote(m, k, t0, tile); };
      if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(mv + it.r0 * 8ull, it.r1 - it.r0, one);
      else stream_mv40<BLOCK, UNROLL>(mv + it.r0 * 40ull, it.r1 - it.r0, one);
    }
    __syncthreads();
    // ---- the masks and the frame's centre count
    row_masks<BLOCK>(tile, k, t0, t1, k.y_lo - 1, crows + 2,
                     [=, &k](int j, int w, int, unsigned long long m) { amask[(size_t)j * k.W + w] = m; });
    if (tid == 0) total[0] = 0u;
    __syncthreads();
    centre_masks<BLOCK>(amask, cmask, total, k, crows);
    __syncthreads();
    const unsigned int n_centres = __builtin_amdgcn_readfirstlane(total[0]);
    if (n_centres < k.min_centres) continue;    // the one uniform branch: the frame does not contribute

    if constexpr (ACC != 0) {
      accumulate<BLOCK, ACC>(amask, cmask, acc_a, acc_c, k, crows);
      if (++pend >= (unsigned int)k.max_run) flush();
    } else {
      if (active) flush_mask<BLOCK>(amask, 1, active + (size_t)s * plane_words + rows_at, k, crows);
      if (centre) flush_mask<BLOCK>(cmask, 0, centre + (size_t)s * plane_words + rows_at, k, crows);
      if (frames && tid == 0) global_add(frames + s, 1u);
    }
  }
  if constexpr (ACC != 0) { if (pend) flush(); }
}

namespace {

template <int REC, int ACC>
hipError_t launch_map(const ActLaunch &L) {
  auto kern = activity_frames_kernel<kActBlock, kActUnroll, REC, ACC>;
  static std::atomic<unsigned long long> ready{0ull};
  const WorkItem *work = static_cast<const WorkItem *>(L.plan_ws);
  const unsigned long long groups = ((unsigned long long)L.n_frames + (unsigned long long)L.k.run - 1ull) / (unsigned long long)L.k.run;
  return launch_over_list(kern, ready, L, groups, [&](unsigned long long g0, unsigned int n) {
    hipLaunchKernelGGL(kern, dim3(n), dim3(kActBlock), L.lds_bytes, L.stream, L.mv, work, (unsigned int)g0, L.n_frames, L.k,
                       L.stream_off, L.n_streams, L.active, L.centre, L.frames);
  });
}

template <int REC>
hipError_t launch_map_acc(const ActLaunch &L) {
  if (L.acc_bits == 32) return launch_map<REC, 32>(L);
  if (L.acc_bits == 16) return launch_map<REC, 16>(L);
  return launch_map<REC, 0>(L);
}

hipError_t clear(unsigned int *out, unsigned long long n, hipStream_t stream) {
  if (!out || n == 0ull) return hipSuccess;
  hipLaunchKernelGGL(activity_clear_kernel, dim3(clear_grid(n)), dim3(256), 0, stream, out, n);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_activity_map(const ActLaunch &L) {
  if (L.rec_bytes != 40 && L.rec_bytes != 8) return hipErrorInvalidValue;
  if (!L.active && !L.centre && !L.frames) return hipErrorInvalidValue;
  if (L.acc_bits != 32 && L.acc_bits != 16 && L.acc_bits != 0) return hipErrorInvalidValue;
  if (L.k.run < 1 || L.k.max_run < 1 || (L.acc_bits == 16 && L.k.max_run > 65535) || L.lds_bytes > L.lds_max ||
      (size_t)L.lds_bytes < act_lds_bytes(L.k.gw, L.k.R, L.acc_bits))
    return hipErrorInvalidValue;
  const unsigned long long plane = (unsigned long long)L.n_streams * (unsigned long long)L.k.gh * (unsigned long long)L.k.gw;
  hipError_t e = clear(L.active, plane, L.stream);
  if (e == hipSuccess) e = clear(L.centre, plane, L.stream);
  if (e == hipSuccess) e = clear(L.frames, L.n_streams, L.stream);
  if (e != hipSuccess) return e;
  if (L.n_frames == 0 || L.n_streams == 0) return hipSuccess;
  if (!L.stream_off || !check_batch_launch(L)) return hipErrorInvalidValue;
  e = plan_work_list(L, nullptr, 0, nullptr, 0);   // flags / centres null: the planner answers nothing itself
  if (e != hipSuccess) return e;
  return L.rec_bytes == 8 ? launch_map_acc<8>(L) : launch_map_acc<40>(L);
}

}  // namespace mtgpu
