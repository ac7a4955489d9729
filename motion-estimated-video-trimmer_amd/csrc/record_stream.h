// record_stream.h — the device helpers every kernel that walks the scan's work list shares: the record loads and
// decodes, the work-list entry load, the scope-aware result store, and — for the kernels derived from the scan (sweep,
// activity, zones, blobs, gmc, gmc_blobs, dir) — the stream search, the tile zero-fill, the plain record streamers, the
// single-threshold vote, the single-level row masks, the centre test of one mask word, and the two passes over a mask
// plane built on it: the centre count and the centre plane.  All `__device__ __forceinline__`: every kernel still compiles its own instantiation, so a
// change here is a change to each of them.  The rule that keeps sharing safe: an edit to this header must leave the
// device assembly of every including translation unit as it was, or be measured for each of them.
// Internal; included after scan_kernels.h; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernels.h"

namespace mtgpu {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef u32x2 u32x2_a8 __attribute__((aligned(8)));
typedef u32x3 u32x3_a4 __attribute__((aligned(4)));
typedef u32x4 u32x4_a16 __attribute__((aligned(16)));

// ---- records.  Bytes 4..15 of a 40-byte record (layout: include/mt_types.h, mt_mv): d.x = w | h<<8 | src_x<<16,
// d.y = src_y | dst_x<<16, d.z = dst_y | pad<<16.  A compact record (REC 8): src_x | src_y<<16, dst_x | dst_y<<16 —
// bytes 6..13 of an AVMotionVector, packed by the host dispatcher (pipe.hip) or mtgpu_pack_records.  All with the
// streaming (nt) hint: every record is read once per pass.
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

// An entry of the work list with ONE 32-byte load — r0, r1 and f arrive together (read field by field the compiler
// fetches f first, tests it, and only then asks for r0 / r1: two memory round trips at the start of every workgroup's
// life instead of one; the list was just written by another kernel, so the first touch of a line comes from beyond
// this XCD's L2).  The address is workgroup-uniform: a scalar load.
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

// ---- results.  One lane, one store.  `sys` (set by the host when the destination is not device memory — the pipe's
// zero-copy staging, a caller's hipHostMalloc'ed buffer): a SYSTEM-scope store (global_store_byte ... sc0 sc1:
// write-through past the XCD's L2, byte-masked) — the kernel then writes pinned host memory over PCIe next to bytes
// that other workgroups, on other XCDs, write into the same line at other times, so no cache on the way may hold the
// line and merge it back later.  Device memory takes the plain store: a write-through store is only acknowledged from
// the memory side, and a workgroup cannot retire before that — measured against round 4's library in one process,
// system-scope stores for EVERY frame cost 1.2 % on 1080p (16 384 flags per launch) and 4 % on 480p (262 144).
template <typename T>
__device__ __forceinline__ void store_result(T *p, T v, int sys) {
  if (sys) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else *p = v;
}
// The one result byte of a frame (`sys`: ScanK::sys_flags) and its centre count (ScanK::sys_centres).
__device__ __forceinline__ void store_flag(unsigned char *flags, unsigned int f, unsigned char v, int sys) {
  store_result(&flags[f], v, sys);
}
__device__ __forceinline__ void store_centres(unsigned int *centres, unsigned int f, unsigned int v, int sys) {
  store_result(&centres[f], v, sys);
}

// ---- a frame's stream: the number of streams that end at or before frame f, i.e. the stream of f where it has one
// (stream s holds frames [stream_off[s], stream_off[s + 1])).  n_streams: f lies behind the last stream.  A frame in
// front of the first stream gets 0, like a frame of stream 0: the caller that minds tests stream_off[0] itself.  Binary
// search on workgroup-uniform values: scalar code.
__device__ __forceinline__ unsigned int stream_of(const unsigned long long *stream_off, unsigned int n_streams, unsigned int f) {
  unsigned int lo = 0u, hi = n_streams;
  while (lo < hi) {
    const unsigned int mid = lo + ((hi - lo) >> 1);
    if (stream_off[mid + 1u] <= (unsigned long long)f) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// ---- the vote tile (tile_words words, a multiple of 4, 16-byte aligned) zeroed with 16-byte stores.  What a kernel
// zeroes behind it (totals, histograms, result words) differs per kernel and stays there.
template <int BLOCK>
__device__ __forceinline__ void zero_tile(unsigned int *tile, int tile_words) {
  u32x4 *c4 = reinterpret_cast<u32x4 *>(tile);
  const int n4 = tile_words >> 2;
  for (int j = threadIdx.x; j < n4; j += BLOCK) c4[j] = (u32x4){0u, 0u, 0u, 0u};
}

// ---- the derived kernels' record streamers.  (The scan's own stream_mv40 / stream_compact / stream_tail, with the
// look-ahead, the spill queue and the bands, are another algorithm and live in scan_kernels.hip.)  `vote`: what one
// record does, a functor on MvFields.  It is taken BY VALUE: a lambda that captures the kernel's parameter block by
// reference is then a few pointers in registers, and the generated code is the code of a streamer written out for that
// kernel; taken by const reference the functor becomes an object in memory to the optimiser (zones: 2 % more
// instructions, up to three more VGPRs).

template <class V>
__device__ __forceinline__ void vote_pair(const u32x4 d, V vote) {
  vote(decode((u32x2){d.x, d.y}));
  vote(decode((u32x2){d.z, d.w}));
}

// 40-byte records [base, base + 40 n): up to 15 head records so that the steps start on a 128-byte line (40 h = -start
// mod 128 has a solution h < 16 whenever the start is 8-byte aligned: 5 * 13 = 1 mod 16), then lane i of a step takes
// record i with UNROLL independent loads in flight, then the rest with every load issued before the first vote.
template <int BLOCK, int UNROLL, class V>
__device__ __forceinline__ void stream_mv40(const unsigned char *base, unsigned long long n, V vote) {
  const int tid = threadIdx.x;
  const unsigned int r = (unsigned int)((uintptr_t)base & 127u);
  if ((r & 7u) == 0u) {
    unsigned long long h = (unsigned long long)((13u * ((16u - (r >> 3)) & 15u)) & 15u);
    h = h < n ? h : n;
    if ((unsigned long long)tid < h) vote(decode(load_fields(base + (unsigned long long)tid * 40ull)));
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
    for (int u = 0; u < UNROLL; ++u) vote(decode(d[u]));
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
      if (ok[u]) vote(decode(d[u]));
  }
}

// Compact records [base, base + 8 n), 8-byte aligned: up to 15 head records one per lane so that the 16-byte pair
// stream starts on a 128-byte line, lane 0 takes an odd last record.
template <int BLOCK, int UNROLL, class V>
__device__ __forceinline__ void stream_compact(const unsigned char *base, unsigned long long n, V vote) {
  const int tid = threadIdx.x;
  constexpr unsigned long long STEP = (unsigned long long)UNROLL * BLOCK;
  constexpr unsigned long long LAST = (unsigned long long)(UNROLL - 1) * BLOCK;
  unsigned long long head = ((0ull - (unsigned long long)(uintptr_t)base) & 127ull) >> 3;
  head = head < n ? head : n;
  const unsigned char *pbase = base + head * 8ull;
  const unsigned long long np = (n - head) >> 1;            // pairs
  if ((unsigned long long)tid < head) vote(decode(load_compact(base + (unsigned long long)tid * 8ull)));
  if (tid == 0 && ((n - head) & 1ull) != 0ull) vote(decode(load_compact(base + (n - 1ull) * 8ull)));
  unsigned long long p = tid;
  for (; p + LAST < np; p += STEP) {
    u32x4 d[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) d[u] = load_pair(pbase + (p + (unsigned long long)u * BLOCK) * 16ull);
    __builtin_amdgcn_sched_barrier(0);   // every load of the step is issued before the first one is consumed
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) vote_pair(d[u], vote);
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
      if (ok[u]) vote_pair(d[u], vote);
  }
}

// One record against one threshold (src/motion_scanner.cpp:246-268): threshold, cell, bounds — the scan's
// keep_and_cell — then one vote.  K: the kernel's parameter block (ActK, ZoneK).  t0: the grid row of tile row 0.
// gy in [y_lo, y_hi) and t0 <= y_lo: the index stays inside the tile.
template <class K>
__device__ __forceinline__ void vote(const MvFields m, const K &k, int t0, unsigned int *tile) {
  const unsigned int dx = (unsigned int)(m.dst_x - m.src_x);   // |dx| <= 65535
  const unsigned int dy = (unsigned int)(m.dst_y - m.src_y);
  // dx*dx < 2^32 exactly; the sum needs 34 bits
  const unsigned long long mag = (unsigned long long)(dx * dx) + (unsigned long long)(dy * dy);
  const int gx = m.dst_x >> k.shift, gy = m.dst_y >> k.shift;
  // 0 <= gx < gw and y_lo <= gy < y_hi (:262) as two unsigned compares (y_hi >= y_lo by construction)
  const bool in = ((unsigned int)gx < (unsigned int)k.gw) & ((unsigned int)(gy - k.y_lo) < (unsigned int)(k.y_hi - k.y_lo));
  if (in && mag >= k.thr) atomicAdd(&tile[(unsigned int)((gy - t0) * k.gw + gx)], 1u);
}

// ---- the 64-bit masks of the active cells (votes >= k.vec_need) of mask rows [0, nrows): mask row j <-> grid row
// g0 + j.  Rows outside the tracked rows [t0, t1) and cells outside the grid are inactive, with vectors_needed == 0 too
// (:282 with vectors_needed == 0: every cell OF THE GRID is active).  Four lanes per (mask row, word), 16 cells each:
// the cells are read in a rotated order (the 64 lanes of a wave hit 64 different LDS banks per step).  One lane of the
// four hands the word to store(j, w, g, m).  (The sweep's form keeps the 16 cells in registers across its vector levels
// and lives in sweep_kernels.hip.)
template <int BLOCK, class K, class S>
__device__ __forceinline__ void row_masks(const unsigned int *cnt, const K &k, int t0, int t1, int g0, int nrows, S store) {
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
    if (tk < ntask && sub == 0) store(j, w, g, m);
  }
}

// ---- the centres (:277-293) of word w of a mask row: mr points at the row (W words), its neighbour rows lie W words
// before and behind it.  Cells x in [1, gw-2] (:280) that are active and have an active 4-neighbour — neighbours across
// word and row boundaries; outside the grid: inactive.  Every neighbour, the carries included, comes from the plane
// handed in.
__device__ __forceinline__ unsigned long long centre_word(const unsigned long long *mr, int w, int W, int gw) {
  const unsigned long long m = mr[w];
  if (m == 0ull) return 0ull;
  const unsigned long long up = mr[w - W], dn = mr[w + W];
  const unsigned long long lcarry = (w > 0) ? (mr[w - 1] >> 63) : 0ull;
  const unsigned long long rcarry = (w + 1 < W) ? (mr[w + 1] << 63) : 0ull;
  const unsigned long long nb = (m << 1) | lcarry | (m >> 1) | rcarry | up | dn;
  const int lo = max(1 - w * 64, 0), hi = min(gw - 1 - w * 64, 64);   // bits [lo,hi)
  unsigned long long valid = 0ull;
  if (hi > lo) {
    valid = (hi >= 64) ? ~0ull : ((1ull << hi) - 1ull);
    valid &= ~((1ull << lo) - 1ull);
  }
  return m & nb & valid;
}

// ---- the centres (:277-293) of one mask plane, one task per (analysed row, word): analysed row r <-> mask row r + 1 of
// amask (crows + 2 rows of W words).  On a masked plane an ignored cell next to a word boundary carries nothing over.
// (The sweep counts per vector level and the activity map keeps every centre word: their passes are their own.)
// The count alone, added to *total:
template <int BLOCK>
__device__ __forceinline__ void count_centres(const unsigned long long *amask, unsigned int *total, int W, int gw, int crows) {
  const int ntask = crows * W;
  for (int tk = threadIdx.x; tk < ntask; tk += BLOCK) {
    const int r = tk / W, w = tk - r * W;
    const unsigned long long *mr = amask + (size_t)(r + 1) * W;
    if (mr[w] == 0ull) continue;                               // no popcount, no add: most words of most frames
    const unsigned int c = (unsigned int)__popcll(centre_word(mr, w, W, gw));
    if (c) atomicAdd(total, c);
  }
}
// The centre words into cpl[0 .. nkeep), nkeep = crows * W, and the count.  Every word is written, the empty ones too.
template <int BLOCK>
__device__ __forceinline__ void centre_plane(const unsigned long long *amask, unsigned long long *cpl, unsigned int *total, int W,
                                             int gw, int nkeep) {
  for (int tk = threadIdx.x; tk < nkeep; tk += BLOCK) {
    const int r = tk / W, w = tk - r * W;
    const unsigned long long c = centre_word(amask + (size_t)(r + 1) * W, w, W, gw);
    cpl[tk] = c;
    if (c) atomicAdd(total, (unsigned int)__popcll(c));
  }
}

}  // namespace mtgpu
