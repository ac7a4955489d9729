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
// The record loads, the streamers, the vote, the row masks, the centre test of a word and the result stores are those
// of record_stream.h, shared with sweep_kernels.hip and activity_kernels.hip and instantiated here with this kernel's
// functors; the launch helpers are those of scan_kernels.h.  A change there must leave this file's device assembly as it
// was.
#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "zones_kernels.hip is written for gfx950 only (wave64, 160 KB LDS)"
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "zones_kernels.h"
#include "record_stream.h"

namespace mtgpu {

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
    s = stream_of(stream_off, n_streams, f);
    if (s >= n_streams) return;                 // a frame in front of the first stream is not told apart: it takes plane 0
  }

  // ---- the keep words of the analysed rows, one contiguous block of the stream's plane.  The first word of every
  // lane is on its way while the tile is zeroed (1080p and 4K: there is no second one).
  const unsigned long long *kp = keep + ((size_t)s * (size_t)k.gh + (size_t)k.y_lo) * (size_t)k.W;
  const int nkeep = crows * k.W;
  const unsigned long long k0 = tid < nkeep ? kp[tid] : 0ull;
  zero_tile<BLOCK>(tile, k.tile_words);
  if (tid < 4) total[tid] = 0u;
  if (tid < nkeep) klds[tid] = k0;
  for (int j = tid + BLOCK; j < nkeep; j += BLOCK) klds[j] = kp[j];
  __syncthreads();
  // ---- the votes (an empty analysed range keeps nothing: nothing to read)
  if (crows > 0) {
    const auto one = [=, &k](const MvFields m) { vote(m, k, t0, tile); };
    if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(mv + me.r0 * 8ull, me.r1 - me.r0, one);
    else stream_mv40<BLOCK, UNROLL>(mv + me.r0 * 40ull, me.r1 - me.r0, one);
  }
  __syncthreads();
  // ---- the masks, then the centre counts: masked, and (one uniform branch) unmasked from the same tile
  const bool want_all = !PIPE && centres_all != nullptr;
  // The word of an analysed row [y_lo, y_hi) is ANDed with the stream's keep word (keep row r <-> grid row y_lo + r)
  // into kmask; umask, where wanted, receives the word as it is.
  unsigned long long *const uplane = want_all ? umask : nullptr;
  row_masks<BLOCK>(tile, k, t0, t1, k.y_lo - 1, crows + 2, [=, &k](int j, int w, int g, unsigned long long m) {
    const bool analysed = g >= k.y_lo && g < k.y_hi;           // then 0 <= g - y_lo < R: inside the staged keep rows
    const unsigned long long kw = analysed ? klds[(size_t)(g - k.y_lo) * k.W + w] : ~0ull;
    kmask[(size_t)j * k.W + w] = m & kw;
    if (uplane) uplane[(size_t)j * k.W + w] = m;
  });
  __syncthreads();
  count_centres<BLOCK>(kmask, &total[0], k.W, k.gw, crows);
  if (want_all) count_centres<BLOCK>(umask, &total[1], k.W, k.gw, crows);
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
  static std::atomic<unsigned long long> ready{0ull};
  const WorkItem *work = static_cast<const WorkItem *>(L.plan_ws);
  return launch_over_list(kern, ready, L, L.n_frames, [&](unsigned long long i0, unsigned int n) {
    hipLaunchKernelGGL(kern, dim3(n), dim3(kZoneBlock), L.lds_bytes, L.stream, L.mv, work, (unsigned int)i0, L.n_frames, L.k,
                       L.stream_off, L.n_streams, L.keep, L.flags, L.centres, L.centres_all, L.sys_flags, L.sys_centres);
  });
}

}  // namespace

hipError_t launch_zone_scan(const ZoneLaunch &L) {
  if (L.n_frames == 0) return hipSuccess;
  if (L.rec_bytes != 40 && L.rec_bytes != 8) return hipErrorInvalidValue;
  if (!L.flags && !L.centres && !L.centres_all) return hipErrorInvalidValue;
  if (L.pipe ? (L.centres_all != nullptr) : (L.sys_flags != 0 || L.sys_centres != 0 || !L.stream_off || L.n_streams == 0))
    return hipErrorInvalidValue;
  if (!L.keep || !check_batch_launch(L) || !check_rows(L.k, L.lds_bytes, L.lds_max, zone_lds_bytes(L.k.gw, L.k.R)))
    return hipErrorInvalidValue;
  return plan_and_launch(
      L, L.pipe, L.flags, L.sys_flags, L.centres, L.sys_centres,
      [&](unsigned int grid) {
        hipLaunchKernelGGL(zones_clear_kernel, dim3(grid), dim3(256), 0, L.stream, L.flags, L.centres, L.centres_all, L.n_frames);
      },
      [&](auto rec, auto pipe) { return launch_frames<rec(), pipe()>(L); });
}

}  // namespace mtgpu
