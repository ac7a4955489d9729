// lanes_kernels.hip — direction planes (include/mtgpu_lanes.h): the direction scan of dir_kernels.hip in which the allow
// byte is the one of the record's destination cell, and the flow map that such a plane is learned from.
//
//   lanes_clear_kernel   zero-fills the non-null outputs ahead of the scan kernel: a frame without side data, and a frame
//                        outside every stream, reads 0 everywhere.
//   lanes_frames_kernel  one workgroup per entry of the scan's work list (plan_frames: the frames with side data, in
//                        stream order).  Surplus workgroups find kNoFrame and leave.
//     stream      with a stream table: s = the number of streams that end at or before frame f, a binary search on
//                 workgroup-uniform values; the frame's plane is plane s.  Without: plane 0 serves every frame.
//     plane       STAGED: rows y_lo .. y_hi - 1 of the plane go to LDS behind the rose words, ahead of the first record.
//                 The source (s gh + y_lo) gw has no alignment beyond one byte (odd gw, s >= 1): up to three head bytes
//                 and up to three tail bytes move alone, the words between them as aligned 32-bit loads and LDS stores —
//                 the LDS copy begins at the source's phase inside a word.  Bytes of other rows are never read.
//                 !STAGED: where those rows do not fit next to the tile, the byte is a plain cached global load.
//     votes       as dir_frames_kernel: zero the tile; stream the records (head peel to a 128-byte line, non-temporal
//                 loads, kLanesUnroll in flight per lane).  Per COUNTING record, behind the branch on the threshold and
//                 the bounds that the vote needs anyway: the sector, ONE byte of the plane at the destination cell, one
//                 shift — then the fire-and-forget `ds_add_u32` of an allowed record.  A record that does not count
//                 costs what it costs in the direction scan.
//     rose        the direction scan's: eight 8-bit fields per lane, summed across each wave once per kLanesChunk records
//                 (flush_rose's scheme), whatever the plane says.
//     masks, centres   row_masks, centre_word through count_centres.
//   Every output element has one writer after the clear: lane 0 of the frame's workgroup, plain vector stores, no global
//   atomics.
//
//   lanes_pipe_kernel    the form for a pipe's staging batch (include/mtgpu_pipe_lanes.h): no clear kernel — the planner
//                        answers the frames without side data — no stream search (ONE plane), no rose array; every
//                        listed frame's workgroup stores the flag and ONE count (the centre count or the sector word) on
//                        the kernel's one exit, through store_flag / store_centres at the outputs' scope.  With a keep
//                        plane the rose counts a record only where the keep bit of its destination cell is set, and the
//                        active plane is the masked one; the keep words wait in the amask rows they are ANDed into.
//
//   flow_clear_kernel    zero-fills the map: the call clears, then counts.
//   flow_frames_kernel   the same work list, stream search and streamers; no tile, no LDS.  Per counting record with a
//                        sector one no-return agent-scope relaxed atomic add of 1 on the word of (stream, sector, cell):
//                        integer adds commute, so the map depends on neither the launch grid nor the order in which
//                        workgroups arrive.  A frame outside every stream counts nowhere.
//
// The record loads, the streamers, the row masks and the centre passes are those of record_stream.h, instantiated here
// with this file's functors; the launch helpers are those of scan_kernels.h.
#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "lanes_kernels.hip is written for gfx950 only (wave64, 160 KB LDS)"
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "lanes_kernels.h"
#include "record_stream.h"

namespace mtgpu {

namespace {

// ---- what a counting record is and where it points (src/motion_scanner.cpp:246-262 and the sector rule of
// include/mtgpu_dir.h, as dir_kernels.hip's dir_vote works them out).
struct Counted {
  bool counts;                   // passes the bounds test and the threshold
  int gx, gy;                    // destination cell
  unsigned int dx, dy;           // displacement, two's complement
};
__device__ __forceinline__ Counted counted(const MvFields m, const LanesK &k) {
  const int sdx = m.dst_x - m.src_x, sdy = m.dst_y - m.src_y;  // |.| <= 65535
  const unsigned int dx = (unsigned int)sdx, dy = (unsigned int)sdy;
  // dx*dx < 2^32 exactly; the sum needs 34 bits
  const unsigned long long mag = (unsigned long long)(dx * dx) + (unsigned long long)(dy * dy);
  const int gx = m.dst_x >> k.shift, gy = m.dst_y >> k.shift;
  // 0 <= gx < gw and y_lo <= gy < y_hi (:262) as two unsigned compares (y_hi >= y_lo by construction)
  const bool in = ((unsigned int)gx < (unsigned int)k.gw) & ((unsigned int)(gy - k.y_lo) < (unsigned int)(k.y_hi - k.y_lo));
  const bool counts = in & (mag >= k.thr);
  return {counts, gx, gy, dx, dy};
}
//   axis tests   e: 12 |dy| <= 5 |dx| (E / W), s: 12 |dx| <= 5 |dy| (S / N); |d| <= 65535, so both products fit 24-bit
//                multiplies.  Both hold only for dx == dy == 0.
//   sector       e: 4 sx; s: 2 + 4 sy; neither: 1 + 4 sy + 2 (sx ^ sy)  (sx, sy: the sign bits: 1, 3, 5, 7 clockwise)
__device__ __forceinline__ unsigned int sector_of(unsigned int dx, unsigned int dy) {
  const int sdx = (int)dx, sdy = (int)dy;
  const unsigned int ax = (unsigned int)(sdx < 0 ? -sdx : sdx), ay = (unsigned int)(sdy < 0 ? -sdy : sdy);
  const bool e = __umul24(12u, ay) <= __umul24(5u, ax), s = __umul24(12u, ax) <= __umul24(5u, ay);
  const unsigned int sx = dx >> 31, sy = dy >> 31;
  const unsigned int diag = 1u | ((sx ^ sy) << 1);
  const unsigned int mid = s ? 2u : diag;
  const unsigned int south = mid | (sy << 2), west = sx << 2;
  return e ? west : south;
}

// ---- one record of the plane scan.  `plane`: row y_lo of the frame's plane — the staged copy in LDS or the plane itself
// in memory; the cell's byte is read behind the branch, so a record that does not count reads nothing.  A counting record
// with a sector goes into the lane's packed rose; a counting record without a sector, or with a sector its cell allows,
// votes.  gy in [y_lo, y_hi) and gx in [0, gw): both indices stay inside the analysed rows.
__device__ __forceinline__ void lanes_vote(const MvFields m, const LanesK &k, int t0, unsigned int *tile, const unsigned char *plane,
                                           unsigned long long &acc) {
  const Counted c = counted(m, k);
  if (c.counts) {
    const unsigned int sec = sector_of(c.dx, c.dy);
    const bool none = (c.dx | c.dy) == 0u;
    const unsigned int allow = (unsigned int)plane[(unsigned int)((c.gy - k.y_lo) * k.gw + c.gx)];
    const unsigned int eff = none ? 0xffu : allow;             // no direction to object to
    acc += (unsigned long long)(none ? 0u : 1u) << (8u * sec);
    if (((eff >> sec) & 1u) != 0u) atomicAdd(&tile[(unsigned int)((c.gy - t0) * k.gw + c.gx)], 1u);
  }
}

// No-return atomic add, agent scope, relaxed: the map is read only after the kernel has completed
// (activity_kernels.hip's global_add).
__device__ __forceinline__ void global_add(unsigned int *p, unsigned int v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- one record of the flow map.  `flow_s`: the eight planes of the frame's stream.
__device__ __forceinline__ void flow_count(const MvFields m, const LanesK &k, unsigned int *flow_s) {
  const Counted c = counted(m, k);
  if (c.counts) {
    const unsigned int sec = sector_of(c.dx, c.dy);
    if ((c.dx | c.dy) != 0u) global_add(flow_s + ((size_t)sec * (size_t)k.gh + (size_t)c.gy) * (size_t)k.gw + (size_t)c.gx, 1u);
  }
}

// ---- sums over a wave, every lane active, and the flush of the lanes' packed rose counters: dir_kernels.hip's scheme
// (DPP inside a row of 16 lanes, four lane reads across the rows; even and odd 8-bit fields spread to 16-bit fields).
template <int CTRL>
__device__ __forceinline__ unsigned int dpp_add(unsigned int v) {
  return v + (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ unsigned int wave_sum(unsigned int v) {
  v = dpp_add<0xB1>(v);
  v = dpp_add<0x4E>(v);
  v = dpp_add<0x141>(v);
  v = dpp_add<0x140>(v);
  return (unsigned int)__builtin_amdgcn_readlane((int)v, 0) + (unsigned int)__builtin_amdgcn_readlane((int)v, 16) +
         (unsigned int)__builtin_amdgcn_readlane((int)v, 32) + (unsigned int)__builtin_amdgcn_readlane((int)v, 48);
}
__device__ __forceinline__ void flush_rose(unsigned long long acc, unsigned int *rose) {
  constexpr unsigned long long kEven = 0x00ff00ff00ff00ffull;
  const unsigned long long ev = acc & kEven, od = (acc >> 8) & kEven;
  const unsigned int e0 = wave_sum((unsigned int)ev), e1 = wave_sum((unsigned int)(ev >> 32));
  const unsigned int o0 = wave_sum((unsigned int)od), o1 = wave_sum((unsigned int)(od >> 32));
  if ((threadIdx.x & 63u) == 0u) {
    const unsigned int n[8] = {e0 & 0xffffu, o0 & 0xffffu, e0 >> 16, o0 >> 16, e1 & 0xffffu, o1 & 0xffffu, e1 >> 16, o1 >> 16};
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (n[j]) atomicAdd(&rose[j], n[j]);
  }
}

// The frame's stream, or n_streams where it has none: behind the last stream, or in front of the first one.
__device__ __forceinline__ unsigned int owning_stream(const unsigned long long *stream_off, unsigned int n_streams, unsigned int f) {
  const unsigned int lo = stream_of(stream_off, n_streams, f);
  return (lo >= n_streams || stream_off[lo] > (unsigned long long)f) ? n_streams : lo;
}

}  // namespace

__global__ __launch_bounds__(256) void lanes_clear_kernel(unsigned char *__restrict__ flags, unsigned int *__restrict__ centres,
                                                          unsigned int *__restrict__ rose, unsigned int n) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull) {
    if (flags) flags[i] = (unsigned char)0;
    if (centres) centres[i] = 0u;
    if (rose) {
#pragma unroll
      for (int j = 0; j < 8; ++j) rose[i * 8ull + j] = 0u;
    }
  }
}

__global__ __launch_bounds__(256) void flow_clear_kernel(unsigned int *__restrict__ flow, unsigned long long n) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull)
    flow[i] = 0u;
}

// Waves per SIMD: as dir_frames_kernel — a workgroup is 16 waves, four per SIMD; a staged 1080p workgroup takes about
// 38 KB of LDS, so the lane limit still decides: two workgroups per CU, eight waves per SIMD and so at most 64 VGPRs.
// stream_off == nullptr: n_streams is not read and plane 0 serves every frame.
template <int BLOCK, int UNROLL, int REC, bool STAGED>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void lanes_frames_kernel(
    const unsigned char *__restrict__ mv, const WorkItem *__restrict__ work, unsigned int item0, unsigned int n_items, LanesK k,
    const unsigned long long *__restrict__ stream_off, unsigned int n_streams, const unsigned char *__restrict__ planes,
    unsigned char *__restrict__ flags, unsigned int *__restrict__ centres, unsigned int *__restrict__ rose) {
  extern __shared__ __attribute__((aligned(16))) unsigned int lds[];
  const unsigned int item = item0 + blockIdx.x;
  if (item >= n_items) return;
  const WorkItem me = load_item(work, item);
  if (me.f == kNoFrame) return;                 // the list has ended (every later entry is past its end too)
  const int tid = threadIdx.x;
  unsigned int *tile = lds;
  unsigned long long *amask = reinterpret_cast<unsigned long long *>(lds + k.tile_words);
  unsigned int *lrose = reinterpret_cast<unsigned int *>(amask + (size_t)(k.R + 2) * k.W);
  unsigned int *total = lrose + 8;
  const int t0 = max(k.y_lo - 1, 0), t1 = min(k.y_hi + 1, k.gh);
  const int crows = k.y_hi - k.y_lo;

  // The frame's stream (workgroup-uniform values: scalar code).  A frame outside every stream keeps the zeros of the clear.
  const unsigned int f = __builtin_amdgcn_readfirstlane(me.f);
  unsigned int s = 0u;
  if (stream_off != nullptr) {
    s = owning_stream(stream_off, n_streams, f);
    if (s >= n_streams) return;
  }
  // rows y_lo .. y_hi - 1 of plane s: crows x gw bytes at any byte address
  const unsigned char *src = planes + ((size_t)s * (size_t)k.gh + (size_t)k.y_lo) * (size_t)k.gw;
  const unsigned char *plane = src;
  // ---- zero the tile, the rose and the total; stage the plane
  zero_tile<BLOCK>(tile, k.tile_words);
  if (tid < 9) lrose[tid] = 0u;                 // the eight rose words and total[0] behind them
  if constexpr (STAGED) {
    const unsigned int nbytes = (unsigned int)(max(crows, 0) * k.gw);
    unsigned int head = (0u - (unsigned int)(uintptr_t)src) & 3u;            // bytes in front of the first aligned word
    head = head < nbytes ? head : nbytes;
    unsigned int *area = total + 4;                                          // 16-byte aligned
    unsigned char *copy = reinterpret_cast<unsigned char *>(area) - head;    // inside total[3], which nobody else touches
    const unsigned int nwords = (nbytes - head) >> 2, tail = (nbytes - head) & 3u;
    if ((unsigned int)tid < head) copy[tid] = src[tid];
    const unsigned int *src4 = reinterpret_cast<const unsigned int *>(src + head);   // 4-byte aligned wherever nwords > 0
    for (unsigned int j = tid; j < nwords; j += BLOCK) area[j] = src4[j];
    const unsigned int done = head + 4u * nwords;
    if ((unsigned int)tid < tail) copy[done + tid] = src[done + tid];
    plane = copy;
  }
  __syncthreads();
  // ---- the votes and the rose (an empty analysed range counts nothing: nothing to read)
  if (crows > 0) {
    for (unsigned long long r = me.r0; r < me.r1; r += kLanesChunk) {    // uniform: one piece unless the frame is huge
      const unsigned long long n = (me.r1 - r) < kLanesChunk ? (me.r1 - r) : kLanesChunk;
      unsigned long long acc = 0ull;
      const auto one = [=, &k, &acc](const MvFields m) { lanes_vote(m, k, t0, tile, plane, acc); };
      if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(mv + r * 8ull, n, one);
      else stream_mv40<BLOCK, UNROLL>(mv + r * 40ull, n, one);
      flush_rose(acc, lrose);
    }
  }
  __syncthreads();
  // ---- the masks, then the centre count
  row_masks<BLOCK>(tile, k, t0, t1, k.y_lo - 1, crows + 2, [=, &k](int j, int w, int g, unsigned long long m) {
    amask[(size_t)j * k.W + w] = m;
  });
  __syncthreads();
  count_centres<BLOCK>(amask, &total[0], k.W, k.gw, crows);
  __syncthreads();
  if (tid == 0) {
    const unsigned int c = total[0];
    if (centres) centres[f] = c;
    if (flags) flags[f] = (unsigned char)(c >= k.clust_need ? 1 : 0);
    if (rose) {
      unsigned int *out = rose + (size_t)f * 8u;
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = lrose[j];
    }
  }
}

// No LDS and a handful of registers: eight waves per SIMD, two workgroups per CU, as the scan kernel above.
template <int BLOCK, int UNROLL, int REC>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void flow_frames_kernel(
    const unsigned char *__restrict__ mv, const WorkItem *__restrict__ work, unsigned int item0, unsigned int n_items, LanesK k,
    const unsigned long long *__restrict__ stream_off, unsigned int n_streams, unsigned int *__restrict__ flow) {
  const unsigned int item = item0 + blockIdx.x;
  if (item >= n_items) return;
  const WorkItem me = load_item(work, item);
  if (me.f == kNoFrame) return;
  const unsigned int f = __builtin_amdgcn_readfirstlane(me.f);
  const unsigned int s = owning_stream(stream_off, n_streams, f);
  if (s >= n_streams || k.y_hi <= k.y_lo) return;
  unsigned int *flow_s = flow + (size_t)s * 8u * (size_t)k.gh * (size_t)k.gw;
  const unsigned long long n = me.r1 - me.r0;
  const auto one = [=, &k](const MvFields m) { flow_count(m, k, flow_s); };
  if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(mv + me.r0 * 8ull, n, one);
  else stream_mv40<BLOCK, UNROLL>(mv + me.r0 * 40ull, n, one);
}

namespace {

// ---- one record of the pipe form (include/mtgpu_pipe_lanes.h).  As lanes_vote; KEEP (under a keep plane): `kl` = the
// staged keep words of the analysed rows (keep row r at kl + r * W).  The keep bit and the plane byte of the destination
// cell are both read behind the branch: a record that does not count reads neither.  A record of a keep-0 cell is in no
// sector of the rose and does not vote (its cell is inactive whatever its votes).
template <bool KEEP>
__device__ __forceinline__ void lanes_pipe_vote(const MvFields m, const LanesK &k, int t0, unsigned int *tile, const unsigned char *plane,
                                                unsigned long long &acc, const unsigned long long *kl) {
  const Counted c = counted(m, k);
  if (c.counts) {
    const unsigned int sec = sector_of(c.dx, c.dy);
    const bool none = (c.dx | c.dy) == 0u;
    const unsigned int allow = (unsigned int)plane[(unsigned int)((c.gy - k.y_lo) * k.gw + c.gx)];
    const unsigned int eff = none ? 0xffu : allow;             // no direction to object to
    if constexpr (KEEP) {
      const bool kept = ((kl[(c.gy - k.y_lo) * k.W + (c.gx >> 6)] >> (c.gx & 63)) & 1ull) != 0ull;
      acc += (unsigned long long)((none | !kept) ? 0u : 1u) << (8u * sec);
      if (kept & (((eff >> sec) & 1u) != 0u)) atomicAdd(&tile[(unsigned int)((c.gy - t0) * k.gw + c.gx)], 1u);
    } else {
      acc += (unsigned long long)(none ? 0u : 1u) << (8u * sec);
      if (((eff >> sec) & 1u) != 0u) atomicAdd(&tile[(unsigned int)((c.gy - t0) * k.gw + c.gx)], 1u);
    }
  }
}

}  // namespace

// The pipe form of lanes_frames_kernel (include/mtgpu_pipe_lanes.h): what dir_frames_kernel<.., PIPE = true> is to the
// direction scan.  No stream search — `plane` is ONE plane (gh x gw bytes) and serves every frame; no rose array; `keep`
// is ONE keep plane (gh x W words) or null.  The flag and the ONE count leave through store_flag / store_centres with
// sys_flags / sys_centres on the kernel's one exit, which an empty analysed range reaches too: a reused pinned block
// holds the previous batch's values, so every listed frame stores.  With report_sectors the count is the sector word lane
// 0 builds from the eight LDS rose words.
//   plane   STAGED: rows y_lo .. y_hi - 1 behind `total`, the copy of lanes_frames_kernel.  The plane starts at an
//           allocation boundary, but y_lo gw is odd for odd gw and odd y_lo: the head and tail byte paths stay live.
//           !STAGED: one cached global byte load per counting record.
//   keep    no LDS of its own: the keep words of the analysed rows wait in the amask rows they will be ANDed into (keep
//           row r <-> mask row r + 1), which are dead until row_masks writes them; the lane that stores a word is the one
//           that reads the keep word under it.  They are alive at the same time as the staged plane bytes, which lie
//           behind `total` and so behind every mask row.  keep == nullptr is a workgroup-uniform branch around the
//           staging and around the masked streamer.
// Waves per SIMD: as lanes_frames_kernel.
template <int BLOCK, int UNROLL, int REC, bool STAGED>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void lanes_pipe_kernel(
    const unsigned char *__restrict__ mv, const WorkItem *__restrict__ work, unsigned int item0, unsigned int n_items, LanesK k,
    const unsigned char *__restrict__ plane1, unsigned char *__restrict__ flags, unsigned int *__restrict__ centres,
    const unsigned long long *__restrict__ keep, int sys_flags, int sys_centres, int report_sectors) {
  extern __shared__ __attribute__((aligned(16))) unsigned int lds[];
  const unsigned int item = item0 + blockIdx.x;
  if (item >= n_items) return;
  const WorkItem me = load_item(work, item);
  if (me.f == kNoFrame) return;                 // the list has ended (every later entry is past its end too)
  const int tid = threadIdx.x;
  unsigned int *tile = lds;
  unsigned long long *amask = reinterpret_cast<unsigned long long *>(lds + k.tile_words);
  unsigned int *lrose = reinterpret_cast<unsigned int *>(amask + (size_t)(k.R + 2) * k.W);
  unsigned int *total = lrose + 8;
  const int t0 = max(k.y_lo - 1, 0), t1 = min(k.y_hi + 1, k.gh);
  const int crows = k.y_hi - k.y_lo;
  const unsigned int f = __builtin_amdgcn_readfirstlane(me.f);
  // rows y_lo .. y_hi - 1 of the plane: crows x gw bytes at any byte address
  const unsigned char *src = plane1 + (size_t)k.y_lo * (size_t)k.gw;
  const unsigned char *plane = src;
  // ---- zero the tile, the rose and the total; stage the plane and the keep rows
  zero_tile<BLOCK>(tile, k.tile_words);
  if (tid < 9) lrose[tid] = 0u;                 // the eight rose words and total[0] behind them
  if constexpr (STAGED) {
    const unsigned int nbytes = (unsigned int)(max(crows, 0) * k.gw);
    unsigned int head = (0u - (unsigned int)(uintptr_t)src) & 3u;            // bytes in front of the first aligned word
    head = head < nbytes ? head : nbytes;
    unsigned int *area = total + 4;                                          // 16-byte aligned
    unsigned char *copy = reinterpret_cast<unsigned char *>(area) - head;    // inside total[3], which nobody else touches
    const unsigned int nwords = (nbytes - head) >> 2, tail = (nbytes - head) & 3u;
    if ((unsigned int)tid < head) copy[tid] = src[tid];
    const unsigned int *src4 = reinterpret_cast<const unsigned int *>(src + head);   // 4-byte aligned wherever nwords > 0
    for (unsigned int j = tid; j < nwords; j += BLOCK) area[j] = src4[j];
    const unsigned int done = head + 4u * nwords;
    if ((unsigned int)tid < tail) copy[done + tid] = src[done + tid];
    plane = copy;
  }
  // the keep words of the analysed rows into mask rows 1 .. crows (crows <= R: inside the (R + 2) x W plane); keep row
  // y_lo + r, r < crows, lies inside the gh x W plane
  if (keep != nullptr) {
    const unsigned long long *kp = keep + (size_t)k.y_lo * (size_t)k.W;
    const int nkeep = crows * k.W;
    for (int j = tid; j < nkeep; j += BLOCK) amask[(size_t)k.W + j] = kp[j];
  }
  // The mask plane's offset and the frame's number wait in VGPRs while the records stream (this form has VGPRs to spare
  // under the 64 of eight waves per SIMD): held in SGPRs they are the values too many there, and the compiler parks
  // them in VGPR lanes itself — SGPR spills, as dir_kernels.hip's pipe form met.  Seen with hipcc 7.2.26015 (AMD clang
  // 22.0.0git, roc-7.2.0): one to three spilled SGPRs per form without this; the results do not depend on it, only the
  // register use does.  With another compiler read the kernels' resource usage again
  // (docs/rounds/r26_pipe_lanes.md has the command line).
  unsigned int tw = (unsigned int)k.tile_words, fv = f;
  asm volatile("" : "+v"(tw));
  asm volatile("" : "+v"(fv));
  __syncthreads();
  // ---- the votes and the rose (an empty analysed range counts nothing: nothing to read)
  if (crows > 0) {
    for (unsigned long long r = me.r0; r < me.r1; r += kLanesChunk) {    // uniform: one piece unless the frame is huge
      const unsigned long long n = (me.r1 - r) < kLanesChunk ? (me.r1 - r) : kLanesChunk;
      unsigned long long acc = 0ull;
      if (keep != nullptr) {
        const unsigned long long *kl = amask + k.W;
        const auto onek = [=, &k, &acc](const MvFields m) { lanes_pipe_vote<true>(m, k, t0, tile, plane, acc, kl); };
        if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(mv + r * 8ull, n, onek);
        else stream_mv40<BLOCK, UNROLL>(mv + r * 40ull, n, onek);
      } else {
        const auto one = [=, &k, &acc](const MvFields m) { lanes_pipe_vote<false>(m, k, t0, tile, plane, acc, nullptr); };
        if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(mv + r * 8ull, n, one);
        else stream_mv40<BLOCK, UNROLL>(mv + r * 40ull, n, one);
      }
      flush_rose(acc, lrose);
    }
  }
  __syncthreads();
  // ---- the masks, then the centre count: an analysed row's word is ANDed with the keep word it overwrites (staged
  // above); halo rows are stored as they come.  The plane, the rose and the total are found again from the offset parked
  // in a VGPR above and from R = max(1, crows), which the launch checks.
  amask = reinterpret_cast<unsigned long long *>(lds + tw);
  lrose = reinterpret_cast<unsigned int *>(amask + (size_t)(max(crows, 1) + 2) * k.W);
  total = lrose + 8;
  const bool masked = keep != nullptr;
  row_masks<BLOCK>(tile, k, t0, t1, k.y_lo - 1, crows + 2, [=, &k](int j, int w, int g, unsigned long long m) {
    unsigned long long *slot = amask + (size_t)j * k.W + w;
    const bool analysed = masked && g >= k.y_lo && g < k.y_hi;
    *slot = analysed ? (m & *slot) : m;
  });
  __syncthreads();
  count_centres<BLOCK>(amask, &total[0], k.W, k.gw, crows);
  __syncthreads();
  if (tid == 0) {                               // the one exit
    const unsigned int c = total[0];
    if (centres) {
      unsigned int word = c;
      if (report_sectors) {
        // present byte | k* << 8 | min(n[k*], 2^21 - 1) << 11; k*: the smallest k whose count is maximal (0: none counts)
        unsigned int present = 0u, best = 0u, kbest = 0u;
#pragma unroll
        for (unsigned int j = 0; j < 8u; ++j) {
          const unsigned int n = lrose[j];
          present |= (n ? 1u : 0u) << j;
          if (n > best) { best = n; kbest = j; }
        }
        word = present | (kbest << 8) | ((best < 0x1fffffu ? best : 0x1fffffu) << 11);
      }
      store_centres(centres, fv, word, sys_centres);
    }
    if (flags) store_flag(flags, fv, (unsigned char)(c >= k.clust_need ? 1 : 0), sys_flags);
  }
}

namespace {

template <int REC, bool STAGED>
hipError_t launch_pipe(const LanesLaunch &L) {
  auto kern = lanes_pipe_kernel<kLanesBlock, kLanesUnroll, REC, STAGED>;
  static std::atomic<unsigned long long> ready{0ull};
  const WorkItem *work = static_cast<const WorkItem *>(L.plan_ws);
  return launch_over_list(kern, ready, L, L.n_frames, [&](unsigned long long i0, unsigned int n) {
    hipLaunchKernelGGL(kern, dim3(n), dim3(kLanesBlock), L.lds_bytes, L.stream, L.mv, work, (unsigned int)i0, L.n_frames, L.k,
                       L.planes, L.flags, L.centres, L.keep, L.sys_flags, L.sys_centres, L.report_sectors);
  });
}

template <int REC, bool STAGED>
hipError_t launch_frames(const LanesLaunch &L) {
  auto kern = lanes_frames_kernel<kLanesBlock, kLanesUnroll, REC, STAGED>;
  static std::atomic<unsigned long long> ready{0ull};
  const WorkItem *work = static_cast<const WorkItem *>(L.plan_ws);
  return launch_over_list(kern, ready, L, L.n_frames, [&](unsigned long long i0, unsigned int n) {
    hipLaunchKernelGGL(kern, dim3(n), dim3(kLanesBlock), L.lds_bytes, L.stream, L.mv, work, (unsigned int)i0, L.n_frames, L.k,
                       L.stream_off, L.n_streams, L.planes, L.flags, L.centres, L.rose);
  });
}

template <int REC>
hipError_t launch_flow(const FlowLaunch &L) {
  auto kern = flow_frames_kernel<kLanesBlock, kLanesUnroll, REC>;
  const WorkItem *work = static_cast<const WorkItem *>(L.plan_ws);
  return launch_chunked(L.n_frames, kGridChunk, [&](unsigned long long i0, unsigned int n) {
    hipLaunchKernelGGL(kern, dim3(n), dim3(kLanesBlock), 0, L.stream, L.mv, work, (unsigned int)i0, L.n_frames, L.k, L.stream_off,
                       L.n_streams, L.flow);
  });
}

}  // namespace

hipError_t launch_lanes_scan(const LanesLaunch &L) {
  if (L.n_frames == 0) return hipSuccess;
  if (L.rec_bytes != 40 && L.rec_bytes != 8) return hipErrorInvalidValue;
  if ((!L.flags && !L.centres && !L.rose) || !L.planes) return hipErrorInvalidValue;
  if (L.stream_off ? L.n_streams == 0 : L.n_streams != 0) return hipErrorInvalidValue;
  // the kernel finds its LDS areas and the plane's rows from the block's layout fields: they must be the grid's
  if (!check_batch_launch(L) || !check_rows(L.k, L.lds_bytes, L.lds_max, lanes_lds_bytes(L.k.gw, L.k.R, L.staged != 0)) ||
      (size_t)L.k.tile_words != dir_tile_words(L.k.gw, L.k.R) || L.k.W != (L.k.gw + 63) / 64 || L.k.y_lo < 0 || L.k.y_hi > L.k.gh ||
      L.k.R != (L.k.y_hi - L.k.y_lo < 1 ? 1 : L.k.y_hi - L.k.y_lo))
    return hipErrorInvalidValue;
  return plan_and_launch(
      L, false, L.flags, 0, L.centres, 0,
      [&](unsigned int grid) {
        hipLaunchKernelGGL(lanes_clear_kernel, dim3(grid), dim3(256), 0, L.stream, L.flags, L.centres, L.rose, L.n_frames);
      },
      [&](auto rec, auto) { return L.staged ? launch_frames<rec(), true>(L) : launch_frames<rec(), false>(L); });
}

hipError_t launch_lanes_pipe(const LanesLaunch &L) {
  if (L.n_frames == 0) return hipSuccess;
  if (L.rec_bytes != 40 && L.rec_bytes != 8) return hipErrorInvalidValue;
  if ((!L.flags && !L.centres) || !L.planes || L.rose || L.stream_off || L.n_streams != 0) return hipErrorInvalidValue;
  if (L.report_sectors && !L.centres) return hipErrorInvalidValue;
  // the kernel finds its LDS areas, the plane's rows and the keep rows from the block's layout fields: they must be the grid's
  if (!check_batch_launch(L) || !check_rows(L.k, L.lds_bytes, L.lds_max, lanes_lds_bytes(L.k.gw, L.k.R, L.staged != 0)) ||
      (size_t)L.k.tile_words != dir_tile_words(L.k.gw, L.k.R) || L.k.W != (L.k.gw + 63) / 64 || L.k.y_lo < 0 || L.k.y_hi > L.k.gh ||
      L.k.R != (L.k.y_hi - L.k.y_lo < 1 ? 1 : L.k.y_hi - L.k.y_lo))
    return hipErrorInvalidValue;
  return plan_and_launch(
      L, true, L.flags, L.sys_flags, L.centres, L.sys_centres, [](unsigned int) {},
      [&](auto rec, auto) { return L.staged ? launch_pipe<rec(), true>(L) : launch_pipe<rec(), false>(L); });
}

hipError_t launch_flow_map(const FlowLaunch &L) {
  if (L.rec_bytes != 40 && L.rec_bytes != 8) return hipErrorInvalidValue;
  if (!L.flow || L.n_streams == 0 || !L.stream_off) return hipErrorInvalidValue;
  if (L.k.gw < 1 || L.k.gh < 1 || L.k.y_lo < 0 || L.k.y_hi > L.k.gh || L.k.y_hi < L.k.y_lo) return hipErrorInvalidValue;
  const unsigned long long words = (unsigned long long)L.n_streams * 8ull * (unsigned long long)L.k.gh * (unsigned long long)L.k.gw;
  hipLaunchKernelGGL(flow_clear_kernel, dim3(clear_grid(words)), dim3(256), 0, L.stream, L.flow, words);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || L.n_frames == 0) return e;
  if (!check_batch_launch(L)) return hipErrorInvalidValue;
  e = plan_work_list(L, nullptr, 0, nullptr, 0);   // flags / centres null: the planner answers nothing itself
  if (e != hipSuccess) return e;
  return L.rec_bytes == 8 ? launch_flow<8>(L) : launch_flow<40>(L);
}

}  // namespace mtgpu
