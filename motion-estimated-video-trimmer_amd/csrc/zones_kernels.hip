// zones_kernels.hip — ignore zones: the centre scan of src/motion_scanner.cpp:242-292 (without the early return) with a
// per-stream keep mask.  On the analysed rows a cell is active iff votes >= vectors_needed (:282) AND its keep bit is
// set; an ignored cell is never a centre and never anybody's neighbour.  Rows outside the analysed range behave as in
// the scan, as neighbour rows with vectors_needed == 0 too.
//
//   zones_clear_kernel    zero-fills the non-null outputs ahead of the scan kernel: a frame without side data, and a
//                         frame behind the last stream, reads 0 everywhere.
//   zones_frames_kernel   one workgroup per entry of the scan's work list (plan_frames: the frames with side data, in
//                         stream order).  Surplus workgroups find kNoFrame and leave.
//     stream      s = the number of streams that end at or before frame f: a binary search on workgroup-uniform values.
//     keep        the stream's keep words of the analysed rows are staged in LDS once per workgroup; the loads are
//                 issued before the tile is zeroed, so their latency lies behind the zero fill.
//     votes       zero the tile; stream the records as the sweep does with one threshold (head peel to a 128-byte
//                 line, non-temporal loads, kZoneUnroll in flight per lane, one fire-and-forget `ds_add_u32` per kept
//                 record).  The mask costs nothing per record.
//     masks       the 64-bit masks of the active cells of every tracked row; the word of an analysed row is ANDed with
//                 the keep word: one AND per 64 cells.  With centres_all the unmasked word goes to a second plane.
//     centres     the shifted-mask neighbour test with carries across word boundaries on the masked plane — the carry
//                 is read from the masked neighbour word — and, with centres_all, once more on the unmasked plane.
//   Every output element has one writer after the clear: lane 0 of the frame's workgroup, plain vector stores, no global
//   atomics.
//
// The pipe form (template argument PIPE; ZoneLaunch::pipe) serves a staging batch of pipe.hip:
//     stream      none: a pipe feeds one recording, plane 0 serves every frame — the search and its loads are compiled out.
//     outputs     flags / centres may be a zero-copy batch's pinned block: lane 0 stores them at system scope when the
//                 launch says so (store_flag / store_centres, the scan's helpers); device memory keeps the plain store.
//     no clear    launch_plan is handed the outputs and answers the frames without side data itself, as in launch_scan:
//                 planning + one kernel.  No centres_all.
//
// Carries its own copies of the few record helpers (as scalar_kernels.hip, sweep_kernels.hip and activity_kernels.hip
// do) and calls launch_plan as it is: no other translation unit's device code changes.
#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "zones_kernels.hip is written for gfx950 only (wave64, 160 KB LDS)"
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "zones_kernels.h"

namespace mtgpu {

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef u32x2 u32x2_a8 __attribute__((aligned(8)));
typedef u32x3 u32x3_a4 __attribute__((aligned(4)));
typedef u32x4 u32x4_a16 __attribute__((aligned(16)));

// The record forms of the scan (scan_kernels.hip): bytes 4..15 of a 40-byte record — d.x = w | h<<8 | src_x<<16,
// d.y = src_y | dst_x<<16, d.z = dst_y | pad<<16 — or a compact record, src_x | src_y<<16, dst_x | dst_y<<16.  All with
// the streaming (nt) hint: every record is read once.
__device__ __forceinline__ u32x3 load_fields(const unsigned char *rec) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x3_a4 *>(rec + 4));
}
__device__ __forceinline__ u32x2 load_compact(const unsigned char *rec) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x2_a8 *>(rec));
}
__device__ __forceinline__ u32x4 load_pair(const unsigned char *two_records) {   // 16-byte aligned
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4_a16 *>(two_records));
}

struct MvFields { int src_x, src_y, dst_x, dst_y; };

__device__ __forceinline__ MvFields decode(const u32x3 d) {
  return {(int)d.x >> 16, (int)(short)(d.y & 0xffffu), (int)d.y >> 16, (int)(short)(d.z & 0xffffu)};
}
__device__ __forceinline__ MvFields decode(const u32x2 d) {
  return {(int)(short)(d.x & 0xffffu), (int)d.x >> 16, (int)(short)(d.y & 0xffffu), (int)d.y >> 16};
}

// An entry of the work list with one 32-byte load (workgroup-uniform address: a scalar load), as the scan reads it.
__device__ __forceinline__ WorkItem load_item(const WorkItem *__restrict__ work, unsigned long long wi) {
  typedef unsigned int u32x8 __attribute__((ext_vector_type(8)));
  const u32x8 raw = *reinterpret_cast<const u32x8 *>(work + wi);
  WorkItem it;
  it.r0 = (unsigned long long)raw[0] | ((unsigned long long)raw[1] << 32);
  it.r1 = (unsigned long long)raw[2] | ((unsigned long long)raw[3] << 32);
  it.f = raw[4];
  it.pad[0] = it.pad[1] = it.pad[2] = 0u;
  return it;
}

// The frame's result byte and its centre count in the pipe form: the scan's store_flag / store_centres
// (scan_kernels.hip).  `sys`: the destination is pinned host memory (a zero-copy staging block) — a system-scope
// write-through store, so that no cache between this workgroup and the host may hold the line; device memory takes the
// plain store.
__device__ __forceinline__ void store_flag(unsigned char *flags, unsigned int f, unsigned char v, int sys) {
  if (sys) __hip_atomic_store(&flags[f], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else flags[f] = v;
}
__device__ __forceinline__ void store_centres(unsigned int *centres, unsigned int f, unsigned int v, int sys) {
  if (sys) __hip_atomic_store(&centres[f], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else centres[f] = v;
}

// One record (src/motion_scanner.cpp:246-268): threshold, cell, bounds — the scan's keep_and_cell — then one vote.
// t0: the grid row of tile row 0.  gy in [y_lo, y_hi) and t0 <= y_lo: the index stays inside the tile.
__device__ __forceinline__ void vote(const MvFields m, const ZoneK &k, int t0, unsigned int *tile) {
  const unsigned int dx = (unsigned int)(m.dst_x - m.src_x);   // |dx| <= 65535
  const unsigned int dy = (unsigned int)(m.dst_y - m.src_y);
  // dx*dx < 2^32 exactly; the sum needs 34 bits
  const unsigned long long mag = (unsigned long long)(dx * dx) + (unsigned long long)(dy * dy);
  const int gx = m.dst_x >> k.shift, gy = m.dst_y >> k.shift;
  // 0 <= gx < gw and y_lo <= gy < y_hi (:262) as two unsigned compares (y_hi >= y_lo by construction)
  const bool in = ((unsigned int)gx < (unsigned int)k.gw) & ((unsigned int)(gy - k.y_lo) < (unsigned int)(k.y_hi - k.y_lo));
  if (in && mag >= k.thr) atomicAdd(&tile[(unsigned int)((gy - t0) * k.gw + gx)], 1u);
}

__device__ __forceinline__ void vote_pair(const u32x4 d, const ZoneK &k, int t0, unsigned int *tile) {
  vote(decode((u32x2){d.x, d.y}), k, t0, tile);
  vote(decode((u32x2){d.z, d.w}), k, t0, tile);
}

// 40-byte records [base, base + 40 n): the sweep's stream_mv40 — up to 15 head records so that the steps start on a
// 128-byte line (40 h = -start mod 128 has a solution h < 16 whenever the start is 8-byte aligned), then lane i of a
// step takes record i with UNROLL independent loads in flight, then the rest with every load issued before the
// first vote.
template <int BLOCK, int UNROLL>
__device__ __forceinline__ void stream_mv40(const unsigned char *base, unsigned long long n, const ZoneK &k, int t0,
                                            unsigned int *tile) {
  const int tid = threadIdx.x;
  const unsigned int r = (unsigned int)((uintptr_t)base & 127u);
  if ((r & 7u) == 0u) {
    unsigned long long h = (unsigned long long)((13u * ((16u - (r >> 3)) & 15u)) & 15u);
    h = h < n ? h : n;
    if ((unsigned long long)tid < h) vote(decode(load_fields(base + (unsigned long long)tid * 40ull)), k, t0, tile);
    base += h * 40ull;
    n -= h;
  }
  unsigned long long i = tid;
  constexpr unsigned long long STEP = (unsigned long long)UNROLL * BLOCK;
  constexpr unsigned long long LAST = (unsigned long long)(UNROLL - 1) * BLOCK;
  for (; i + LAST < n; i += STEP) {
    u32x3 d[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) d[u] = load_fields(base + (i + (unsigned long long)u * BLOCK) * 40ull);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) vote(decode(d[u]), k, t0, tile);
  }
  if (i < n) {
    u32x3 d[UNROLL];
    bool ok[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const unsigned long long q = i + (unsigned long long)u * BLOCK;
      ok[u] = q < n;
      if (ok[u]) d[u] = load_fields(base + q * 40ull);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
      if (ok[u]) vote(decode(d[u]), k, t0, tile);
  }
}

// Compact records [base, base + 8 n), 8-byte aligned: the sweep's stream_compact — up to 15 head records one per lane
// so that the 16-byte pair stream starts on a 128-byte line, lane 0 takes an odd last record.
template <int BLOCK, int UNROLL>
__device__ __forceinline__ void stream_compact(const unsigned char *base, unsigned long long n, const ZoneK &k, int t0,
                                               unsigned int *tile) {
  const int tid = threadIdx.x;
  constexpr unsigned long long STEP = (unsigned long long)UNROLL * BLOCK;
  constexpr unsigned long long LAST = (unsigned long long)(UNROLL - 1) * BLOCK;
  unsigned long long head = ((0ull - (unsigned long long)(uintptr_t)base) & 127ull) >> 3;
  head = head < n ? head : n;
  const unsigned char *pbase = base + head * 8ull;
  const unsigned long long np = (n - head) >> 1;            // pairs
  if ((unsigned long long)tid < head) vote(decode(load_compact(base + (unsigned long long)tid * 8ull)), k, t0, tile);
  if (tid == 0 && ((n - head) & 1ull) != 0ull) vote(decode(load_compact(base + (n - 1ull) * 8ull)), k, t0, tile);
  unsigned long long p = tid;
  for (; p + LAST < np; p += STEP) {
    u32x4 d[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) d[u] = load_pair(pbase + (p + (unsigned long long)u * BLOCK) * 16ull);
    __builtin_amdgcn_sched_barrier(0);   // every load of the step is issued before the first one is consumed
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) vote_pair(d[u], k, t0, tile);
  }
  if (p < np) {
    u32x4 d[UNROLL];
    bool ok[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const unsigned long long q = p + (unsigned long long)u * BLOCK;
      ok[u] = q < np;
      if (ok[u]) d[u] = load_pair(pbase + q * 16ull);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
      if (ok[u]) vote_pair(d[u], k, t0, tile);
  }
}

// ---- the 64-bit masks of the active cells of mask rows [0, nrows): mask row j <-> grid row g0 + j.  Rows outside the
// tracked rows [t0, t1) and cells outside the grid are inactive, with vectors_needed == 0 too (:282 with
// vectors_needed == 0: every cell OF THE GRID is active).  Four lanes per (mask row, word), 16 cells each, as the
// sweep's row_masks: the cells are read in a rotated order (the 64 lanes of a wave hit 64 different LDS banks per step).
// The word of an analysed row [y_lo, y_hi) is ANDed with the stream's keep word (keep row r <-> grid row y_lo + r) into
// kmask; umask, where not null, receives the word as it is.
template <int BLOCK>
__device__ __forceinline__ void row_masks(const unsigned int *cnt, const unsigned long long *keep, unsigned long long *kmask,
                                          unsigned long long *umask, const ZoneK &k, int t0, int t1, int g0, int nrows) {
  const int tid = threadIdx.x, W = k.W;
  const int lane = tid & 63;
  const int sub = lane & 3, rot = (lane >> 2) & 15;
  const int ntask = nrows * W * 4;
  for (int t0q = 0; t0q < ntask; t0q += BLOCK) {               // uniform trip count: shuffles below
    const int tk = t0q + tid;
    const int tw = tk >> 2;
    const int j = tw / W, w = tw - j * W;
    const int g = g0 + j;
    const int ncell = min(64, k.gw - w * 64) - sub * 16;       // cells of this lane's quarter inside the grid
    const bool live = tk < ntask && g >= t0 && g < t1 && ncell > 0;
    const int last = min(ncell, 16) - 1;
    unsigned int q = 0u;                                       // bit u: the cell read u-th, i.e. cell (u + rot) & 15
    if (live) {
      const unsigned int *row = cnt + (size_t)(g - t0) * k.gw + w * 64 + sub * 16;
#pragma unroll
      for (int u = 0; u < 16; ++u) q |= (row[min((u + rot) & 15, last)] >= k.vec_need ? 1u : 0u) << u;   // always inside the row
    }
    const unsigned int valid = live ? ((2u << last) - 1u) : 0u;               // bits 0 .. last
    q = ((q << rot) | (q >> (16 - rot))) & 0xffffu & valid;    // rotate the 16 bits into cell order
    unsigned long long m = (unsigned long long)q << (sub * 16);
    m |= __shfl_xor(m, 1);
    m |= __shfl_xor(m, 2);
    if (tk < ntask && sub == 0) {
      const bool analysed = g >= k.y_lo && g < k.y_hi;         // then 0 <= g - y_lo < R: inside the staged keep rows
      const unsigned long long kw = analysed ? keep[(size_t)(g - k.y_lo) * W + w] : ~0ull;
      kmask[(size_t)j * W + w] = m & kw;
      if (umask) umask[(size_t)j * W + w] = m;
    }
  }
}

// ---- the centres (:277-293), one task per (analysed row, word): analysed row r <-> mask row r + 1; x in [1, gw-2]
// (:280); neighbours across word and row boundaries; outside the grid: inactive.  The sweep's count_centres with one
// level.  Every neighbour, the carries included, comes from the plane handed in: on the masked plane an ignored cell
// next to a word boundary carries nothing over.
template <int BLOCK>
__device__ __forceinline__ void count_centres(const unsigned long long *amask, unsigned int *total, const ZoneK &k, int crows) {
  const int W = k.W;
  const int ntask = crows * W;
  for (int tk = threadIdx.x; tk < ntask; tk += BLOCK) {
    const int r = tk / W, w = tk - r * W;
    const unsigned long long *mr = amask + (size_t)(r + 1) * W;
    const unsigned long long m = mr[w];
    if (m == 0ull) continue;
    const unsigned long long up = mr[w - W], dn = mr[w + W];
    const unsigned long long lcarry = (w > 0) ? (mr[w - 1] >> 63) : 0ull;
    const unsigned long long rcarry = (w + 1 < W) ? (mr[w + 1] << 63) : 0ull;
    const unsigned long long nb = (m << 1) | lcarry | (m >> 1) | rcarry | up | dn;
    const int lo = max(1 - w * 64, 0), hi = min(k.gw - 1 - w * 64, 64);   // bits [lo,hi)
    unsigned long long valid = 0ull;
    if (hi > lo) {
      valid = (hi >= 64) ? ~0ull : ((1ull << hi) - 1ull);
      valid &= ~((1ull << lo) - 1ull);
    }
    const unsigned int c = (unsigned int)__popcll(m & nb & valid);
    if (c) atomicAdd(total, c);
  }
}

}  // namespace

__global__ __launch_bounds__(256) void zones_clear_kernel(unsigned char *__restrict__ flags, unsigned int *__restrict__ centres,
                                                          unsigned int *__restrict__ centres_all, unsigned int n) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull) {
    if (flags) flags[i] = (unsigned char)0;
    if (centres) centres[i] = 0u;
    if (centres_all) centres_all[i] = 0u;
  }
}

// Waves per SIMD: a workgroup is 16 waves, four per SIMD.  A 1080p workgroup takes about 36 KB of LDS, so the lane
// limit (2048 per CU), not LDS, decides: two workgroups per CU, eight waves per SIMD and so at most 64 VGPRs.  The 4K
// workgroup (about 141 KB) sits alone on its CU and loses nothing by the same limit.
// PIPE: the form for a pipe's staging batch — stream_off / n_streams / centres_all are not read (null / 1 / null), plane 0
// of `keep` serves every frame, and the two results leave through store_flag / store_centres with sys_flags /
// sys_centres.  !PIPE: sys_* are not read (0).
template <int BLOCK, int UNROLL, int REC, bool PIPE>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void zones_frames_kernel(
    const unsigned char *__restrict__ mv, const WorkItem *__restrict__ work, unsigned int item0, unsigned int n_items, ZoneK k,
    const unsigned long long *__restrict__ stream_off, unsigned int n_streams, const unsigned long long *__restrict__ keep,
    unsigned char *__restrict__ flags, unsigned int *__restrict__ centres, unsigned int *__restrict__ centres_all, int sys_flags,
    int sys_centres) {
  extern __shared__ __attribute__((aligned(16))) unsigned int lds[];
  const unsigned int item = item0 + blockIdx.x;
  if (item >= n_items) return;
  const WorkItem me = load_item(work, item);
  if (me.f == kNoFrame) return;                 // the list has ended (every later entry is past its end too)
  const int tid = threadIdx.x;
  unsigned int *tile = lds;
  unsigned long long *klds = reinterpret_cast<unsigned long long *>(lds + k.tile_words);
  unsigned long long *kmask = klds + (size_t)k.R * k.W;
  unsigned long long *umask = kmask + (size_t)(k.R + 2) * k.W;
  unsigned int *total = reinterpret_cast<unsigned int *>(umask + (size_t)(k.R + 2) * k.W);
  const int t0 = max(k.y_lo - 1, 0), t1 = min(k.y_hi + 1, k.gh);
  const int crows = k.y_hi - k.y_lo;

  // The frame's stream: s = the number of streams that end at or before frame f (binary search, workgroup-uniform
  // values: scalar code).  s == n_streams: the frame lies behind the last stream and keeps the zeros of the clear.
  const unsigned int f = __builtin_amdgcn_readfirstlane(me.f);
  unsigned int s = 0u;
  if constexpr (!PIPE) {
    unsigned int lo = 0u, hi = n_streams;
    while (lo < hi) {
      const unsigned int mid = lo + ((hi - lo) >> 1);
      if (stream_off[mid + 1u] <= (unsigned long long)f) lo = mid + 1u; else hi = mid;
    }
    s = lo;
    if (s >= n_streams) return;
  }

  // ---- the keep words of the analysed rows, one contiguous block of the stream's plane.  The first word of every
  // lane is on its way while the tile is zeroed (1080p and 4K: there is no second one).
  const unsigned long long *kp = keep + ((size_t)s * (size_t)k.gh + (size_t)k.y_lo) * (size_t)k.W;
  const int nkeep = crows * k.W;
  const unsigned long long k0 = tid < nkeep ? kp[tid] : 0ull;
  // ---- zero the tile
  {
    u32x4 *c4 = reinterpret_cast<u32x4 *>(tile);
    const int n4 = k.tile_words >> 2;
    for (int j = tid; j < n4; j += BLOCK) c4[j] = (u32x4){0u, 0u, 0u, 0u};
    if (tid < 4) total[tid] = 0u;
  }
  if (tid < nkeep) klds[tid] = k0;
  for (int j = tid + BLOCK; j < nkeep; j += BLOCK) klds[j] = kp[j];
  __syncthreads();
  // ---- the votes (an empty analysed range keeps nothing: nothing to read)
  if (crows > 0) {
    if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(mv + me.r0 * 8ull, me.r1 - me.r0, k, t0, tile);
    else stream_mv40<BLOCK, UNROLL>(mv + me.r0 * 40ull, me.r1 - me.r0, k, t0, tile);
  }
  __syncthreads();
  // ---- the masks, then the centre counts: masked, and (one uniform branch) unmasked from the same tile
  const bool want_all = !PIPE && centres_all != nullptr;
  row_masks<BLOCK>(tile, klds, kmask, want_all ? umask : nullptr, k, t0, t1, k.y_lo - 1, crows + 2);
  __syncthreads();
  count_centres<BLOCK>(kmask, &total[0], k, crows);
  if (want_all) count_centres<BLOCK>(umask, &total[1], k, crows);
  __syncthreads();
  if (tid == 0) {
    const unsigned int c = total[0];
    if constexpr (PIPE) {
      if (centres) store_centres(centres, f, c, sys_centres);
      if (flags) store_flag(flags, f, (unsigned char)(c >= k.clust_need ? 1 : 0), sys_flags);
    } else {
      if (centres) centres[f] = c;
      if (flags) flags[f] = (unsigned char)(c >= k.clust_need ? 1 : 0);
      if (want_all) centres_all[f] = total[1];
    }
  }
}

namespace {

template <int REC, bool PIPE>
hipError_t launch_frames(const ZoneLaunch &L) {
  auto kern = zones_frames_kernel<kZoneBlock, kZoneUnroll, REC, PIPE>;
  // Dynamic-LDS ceiling: set once per instantiation and device to the device maximum (scan_kernels.hip, launch_one)
  static std::atomic<unsigned long long> ready{0ull};
  const unsigned long long bit = 1ull << (L.device & 63);
  if ((ready.load(std::memory_order_acquire) & bit) == 0ull) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, L.lds_max);
    if (e != hipSuccess) return e;
    ready.fetch_or(bit, std::memory_order_release);
  }
  const WorkItem *work = static_cast<const WorkItem *>(L.plan_ws);
  const unsigned long long chunk = 1ull << 30;             // workgroups per launch: grid.x stays < 2^31
  for (unsigned long long i0 = 0; i0 < L.n_frames; i0 += chunk) {
    const unsigned long long left = (unsigned long long)L.n_frames - i0;
    hipLaunchKernelGGL(kern, dim3((unsigned int)(left < chunk ? left : chunk)), dim3(kZoneBlock), L.lds_bytes, L.stream, L.mv,
                       work, (unsigned int)i0, L.n_frames, L.k, L.stream_off, L.n_streams, L.keep, L.flags, L.centres,
                       L.centres_all, L.sys_flags, L.sys_centres);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_zone_scan(const ZoneLaunch &L) {
  if (L.n_frames == 0) return hipSuccess;
  if (L.rec_bytes != 40 && L.rec_bytes != 8) return hipErrorInvalidValue;
  if (!L.flags && !L.centres && !L.centres_all) return hipErrorInvalidValue;
  if (L.pipe ? (L.centres_all != nullptr) : (L.sys_flags != 0 || L.sys_centres != 0 || !L.stream_off || L.n_streams == 0))
    return hipErrorInvalidValue;
  if (!L.frame_off || !L.keep || !L.plan_ws || ((uintptr_t)L.plan_ws & 31u) != 0u ||
      L.rebase > L.n_records)
    return hipErrorInvalidValue;
  if (L.k.R < 1 || L.k.y_hi < L.k.y_lo || L.k.R < L.k.y_hi - L.k.y_lo || L.lds_bytes > L.lds_max ||
      (size_t)L.lds_bytes < zone_lds_bytes(L.k.gw, L.k.R))
    return hipErrorInvalidValue;
  if (L.pipe) {
    // The planner is handed the outputs and answers every frame without side data itself (plan_scatter_kernel, at the
    // outputs' scope), as in launch_scan: no clear kernel — planning + one kernel.
    WorkItem *work = static_cast<WorkItem *>(L.plan_ws);
    unsigned int *blk_cnt = reinterpret_cast<unsigned int *>(work + (size_t)L.n_frames + 1u);
    hipError_t e = launch_plan(L.frame_off, L.has_sd, L.n_records, L.rebase, L.n_frames, L.flags, L.sys_flags, L.centres,
                               L.sys_centres, work, blk_cnt, L.stream);
    if (e != hipSuccess) return e;
    if (L.ev_planned && (e = hipEventRecord(L.ev_planned, L.stream)) != hipSuccess) return e;
    return L.rec_bytes == 8 ? launch_frames<8, true>(L) : launch_frames<40, true>(L);
  }
  {
    const unsigned long long blocks = ((unsigned long long)L.n_frames + 255ull) / 256ull;
    hipLaunchKernelGGL(zones_clear_kernel, dim3((unsigned int)(blocks < 1024ull ? blocks : 1024ull)), dim3(256), 0, L.stream,
                       L.flags, L.centres, L.centres_all, L.n_frames);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  WorkItem *work = static_cast<WorkItem *>(L.plan_ws);
  unsigned int *blk_cnt = reinterpret_cast<unsigned int *>(work + (size_t)L.n_frames + 1u);
  // flags / centres null: the planner answers nothing itself (the outputs are zero already)
  hipError_t e = launch_plan(L.frame_off, L.has_sd, L.n_records, L.rebase, L.n_frames, nullptr, 0, nullptr, 0, work, blk_cnt,
                             L.stream);
  if (e != hipSuccess) return e;
  if (L.ev_planned && (e = hipEventRecord(L.ev_planned, L.stream)) != hipSuccess) return e;
  return L.rec_bytes == 8 ? launch_frames<8, false>(L) : launch_frames<40, false>(L);
}

}  // namespace mtgpu
