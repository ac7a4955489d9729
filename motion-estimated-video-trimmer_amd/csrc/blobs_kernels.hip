// blobs_kernels.hip — motion blobs: the 4-connected components of a frame's centre cells.  The centre test is that of
// src/motion_scanner.cpp:272-294 (without the early return), on the active cells of mtgpu_scan_centres_device or, with
// a keep mask, of mtgpu_scan_zones_device; what is new is the labelling of the centre plane in LDS.
//
//   blobs_clear_kernel    fills the non-null outputs ahead of the scan kernel with the answer of a frame without a blob
//                         (0 everywhere, an all-0xFFFF box): a frame without side data, and a frame behind the last
//                         stream, has no workgroup.
//   blobs_frames_kernel   one workgroup per entry of the scan's work list, as zones_frames_kernel:
//     stream, keep, votes, masks   as there (no mask: every keep word reads as ones, no stream lookup)
//     centres     centre_word() of every (analysed row, word) into a centre plane — it takes the place of the staged
//                 keep words, which are dead by then — and the frame's centre count.
//     no centre   a workgroup-uniform test: lane 0 stores the zeros and the workgroup ends.  Most frames of a
//                 surveillance stream end here, at the cost of the centre scan.
//     labels      the vote tile is dead once the masks exist: word r * gw + x of it is the label of centre (x, y_lo + r).
//                 A root holds kRoot | (cells - 1), every other cell the index of a cell of its component with a smaller
//                 index.  Union-find, no round-by-round propagation:
//         init      a cell points at the first cell of its horizontal run (bit scan over the row's words): a run is
//                   one tree of depth 1 before the first union
//         unite     one union per segment in which two runs of neighbouring rows overlap: find both roots, link the
//                   larger index to the smaller with one LDS atomicMin, go on with whatever the atomic displaced.
//                   Lock-free, no barrier inside, ends when both cells have one root.
//         flatten   every cell finds its root, stores it, and adds itself to the root's count — one LDS add per
//                   (wave, distinct root): a wave owns one 64-cell word of one row, which is rarely more than one blob.
//         winner    roots: one add for the number of blobs, one 64-bit atomicMax on cells << 32 | ~root — the root is
//                   the smallest cell index of its blob, so the larger key among equal sizes is the blob that holds the
//                   smaller y * gw + x.
//         box       LDS min / max over the winner's cells, one set of four per wave that holds any.
//     Every loop with a barrier inside has a trip count computed from workgroup-uniform values; no loop has an
//     iteration cap: find walks strictly decreasing indices, unite ends when the roots are equal.
//   Every output element has one writer after the clear: lane 0 of the frame's workgroup, plain vector stores, no global
//   atomics.
//
// The pipe form (template argument PIPE; BlobLaunch::pipe) serves a staging batch of pipe.hip, as zones_frames_kernel's:
//     stream      none: a pipe feeds one recording, plane 0 of `keep` serves every frame — the search and its loads are
//                 compiled out.  keep == nullptr is still "no mask".
//     outputs     flags and ONE count array (centres or largest, the other null; no blobs, no box: the staging block has
//                 one count array).  Either may be a zero-copy batch's pinned block: lane 0 stores them at system scope
//                 when the launch says so (store_flag / store_centres of record_stream.h) — on BOTH exits, the early
//                 `no centre` one too: in a reused pinned block it overwrites the previous batch's values.
//     box         the boxed pipe form (REC | kRecBoxed; MT_LAYOUT_BOXES, include/mtgpu_pipe_boxes.h) also stores the
//                 winner's box, on the final exit only: one 8-byte store at the flags' scope.  The early exit and the
//                 planner store none — a box is specified where the flag is set.
//     no clear    launch_plan is handed the outputs and answers the frames without side data itself, as in launch_scan:
//                 planning + one kernel.
//
// The record loads, the stream search, the streamers, the vote, the row masks and the centre plane are those of
// record_stream.h, the five labelling passes those of blob_label.h (one text, shared with gmc_blobs_kernels.hip); the
// launch helpers are those of scan_kernels.h.
#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "blobs_kernels.hip is written for gfx950 only (wave64, 160 KB LDS)"
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "blobs_kernels.h"
#include "record_stream.h"
#include "blob_label.h"

namespace mtgpu {

__global__ __launch_bounds__(256) void blobs_clear_kernel(unsigned char *__restrict__ flags, unsigned int *__restrict__ centres,
                                                          unsigned int *__restrict__ blobs, unsigned int *__restrict__ largest,
                                                          BlobBox *__restrict__ box, unsigned int n) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull) {
    if (flags) flags[i] = (unsigned char)0;
    if (centres) centres[i] = 0u;
    if (blobs) blobs[i] = 0u;
    if (largest) largest[i] = 0u;
    if (box) box[i] = BlobBox{0xffffu, 0xffffu, 0xffffu, 0xffffu};
  }
}

// Waves per SIMD: as zones_frames_kernel — a 1080p workgroup takes about 35 KB of LDS, two workgroups of 16 waves share
// a CU, eight waves per SIMD and so at most 64 VGPRs; the 4K workgroup sits alone on its CU.
// PIPE: the form for a pipe's staging batch — stream_off / n_streams / blobs / box are not read (null / 0 / null / null),
// plane 0 of `keep` serves every frame, at most one of centres / largest is given, and the results leave through
// store_flag / store_centres with sys_flags / sys_centres (sys_centres: whichever count is given).  !PIPE: sys_* are not
// read (0).
// REC: 8 or 40, the bytes per record; | kRecBoxed (blobs_kernels.h): the boxed pipe form (MT_LAYOUT_BOXES,
// include/mtgpu_pipe_boxes.h) — `box` is the batch's box array, 8-byte aligned, and the final exit stores the winner's box
// there.  The early exit and the planner store no box: it is specified only where the flag is set.
template <int BLOCK, int UNROLL, int REC, bool PIPE>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void blobs_frames_kernel(
    const unsigned char *__restrict__ mv, const WorkItem *__restrict__ work, unsigned int item0, unsigned int n_items, BlobK k,
    const unsigned long long *__restrict__ stream_off, unsigned int n_streams, const unsigned long long *__restrict__ keep,
    unsigned char *__restrict__ flags, unsigned int *__restrict__ centres, unsigned int *__restrict__ blobs,
    unsigned int *__restrict__ largest, BlobBox *__restrict__ box, int sys_flags, int sys_centres) {
  static_assert(BLOCK % 64 == 0, "a wave owns one word of the centre plane");
  constexpr bool BOXED = (REC & kRecBoxed) != 0;     // the boxed pipe form: `box` is the batch's box array
  constexpr int RB = REC & ~kRecBoxed;               // bytes per record
  static_assert((RB == 8 || RB == 40) && (PIPE || !BOXED), "8 or 40 bytes per record; the boxed form is a pipe form");
  extern __shared__ __attribute__((aligned(16))) unsigned int lds[];
  const unsigned int item = item0 + blockIdx.x;
  if (item >= n_items) return;
  const WorkItem me = load_item(work, item);
  if (me.f == kNoFrame) return;                 // the list has ended (every later entry is past its end too)
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  unsigned int *tile = lds;
  unsigned long long *klds = reinterpret_cast<unsigned long long *>(lds + k.tile_words);
  unsigned long long *amask = klds + (size_t)k.R * k.W;
  unsigned int *total = reinterpret_cast<unsigned int *>(amask + (size_t)(k.R + 2) * k.W);
  const int t0 = max(k.y_lo - 1, 0), t1 = min(k.y_hi + 1, k.gh);
  const int crows = k.y_hi - k.y_lo;
  const int W = k.W, gw = k.gw;

  // The frame's stream, under a mask only: s = the number of streams that end at or before frame f (binary search on
  // workgroup-uniform values).  s == n_streams: the frame lies behind the last stream and keeps what the clear wrote.
  const unsigned int f = __builtin_amdgcn_readfirstlane(me.f);
  const bool masked = keep != nullptr;
  unsigned int s = 0u;
  if (!PIPE && masked) {
    s = stream_of(stream_off, n_streams, f);
    if (s >= n_streams) return;                 // a frame in front of the first stream is not told apart: it takes plane 0
  }

  // ---- the keep words of the analysed rows (no mask: ones), the first word of a lane on its way while the tile is zeroed
  const int nkeep = crows * W;
  const unsigned long long *kp = masked ? keep + ((size_t)s * (size_t)k.gh + (size_t)k.y_lo) * (size_t)W : nullptr;
  const unsigned long long k0 = (masked && tid < nkeep) ? kp[tid] : ~0ull;
  zero_tile<BLOCK>(tile, k.tile_words);
  if (tid < 8) total[tid] = (tid == 4 || tid == 5) ? 0xffffffffu : 0u;   // [4], [5]: minima
  if (tid < nkeep) klds[tid] = k0;
  for (int j = tid + BLOCK; j < nkeep; j += BLOCK) klds[j] = masked ? kp[j] : ~0ull;
  __syncthreads();
  // ---- the votes (an empty analysed range keeps nothing: nothing to read)
  if (crows > 0) {
    const auto one = [=, &k](const MvFields m) { vote(m, k, t0, tile); };
    if constexpr (RB == 8) stream_compact<BLOCK, UNROLL>(mv + me.r0 * 8ull, me.r1 - me.r0, one);
    else stream_mv40<BLOCK, UNROLL>(mv + me.r0 * 40ull, me.r1 - me.r0, one);
  }
  __syncthreads();
  // ---- the masks: the word of an analysed row [y_lo, y_hi) is ANDed with the keep word (keep row r <-> grid row y_lo + r)
  row_masks<BLOCK>(tile, k, t0, t1, k.y_lo - 1, crows + 2, [=, &k](int j, int w, int g, unsigned long long m) {
    const bool analysed = g >= k.y_lo && g < k.y_hi;           // then 0 <= g - y_lo < R: inside the staged keep rows
    const unsigned long long kw = analysed ? klds[(size_t)(g - k.y_lo) * k.W + w] : ~0ull;
    amask[(size_t)j * k.W + w] = m & kw;
  });
  __syncthreads();
  // ---- the centre plane (over the keep words, dead now) and the count.  Every word is written, the empty ones too.
  unsigned long long *cpl = klds;
  centre_plane<BLOCK>(amask, cpl, &total[0], W, gw, nkeep);
  __syncthreads();
  const unsigned int ncentres = total[0];
  if (ncentres == 0u) {                                       // workgroup-uniform: most frames of most streams
    if (tid == 0) {
      if constexpr (PIPE) {                                     // a reused pinned block holds the previous batch's values
        if (centres) store_centres(centres, f, 0u, sys_centres);
        if (largest) store_centres(largest, f, 0u, sys_centres);
        if (flags) store_flag(flags, f, (unsigned char)0, sys_flags);
      } else {
        if (centres) centres[f] = 0u;
        if (blobs) blobs[f] = 0u;
        if (largest) largest[f] = 0u;
        if (box) box[f] = BlobBox{0xffffu, 0xffffu, 0xffffu, 0xffffu};
        if (flags) flags[f] = (unsigned char)0;
      }
    }
    return;
  }

  // ---- labels.  L[r * gw + x], r < crows <= R: inside the tile's (R + 2) * gw words.
  unsigned int *L = tile;
  // The five passes of blob_label.h, a barrier behind each.
  blob_label::init<BLOCK>(cpl, crows, W, gw, L, lane);
  __syncthreads();
  blob_label::unite_rows<BLOCK>(cpl, crows, W, gw, L, lane);
  __syncthreads();
  blob_label::flatten<BLOCK>(cpl, crows, W, gw, L, lane);
  __syncthreads();
  blob_label::winner<BLOCK>(cpl, crows, W, gw, L, total, lane);
  __syncthreads();
  const unsigned long long key = *reinterpret_cast<const unsigned long long *>(total + 2);
  // In the PIPE form without BOXED nothing reads the box, and in every PIPE form nothing reads the blob count total[1]:
  // both are computed all the same, on purpose — the five passes are those of the resident form, unchanged.
  blob_label::box<BLOCK>(cpl, crows, W, gw, L, total, 0xffffffffu - (unsigned int)(key & 0xffffffffull), lane);
  __syncthreads();
  if (tid == 0) {
    const unsigned int big = (unsigned int)(key >> 32);
    if constexpr (PIPE) {
      if (centres) store_centres(centres, f, ncentres, sys_centres);
      if (largest) store_centres(largest, f, big, sys_centres);
      if constexpr (BOXED)                                      // ONE 8-byte store, at the flags' scope: the same block
        store_result(reinterpret_cast<unsigned long long *>(box) + f, pack_box(total[4], total[5] + (unsigned int)k.y_lo, total[6],
                                                                               total[7] + (unsigned int)k.y_lo), sys_flags);
      if (flags) store_flag(flags, f, (unsigned char)((ncentres >= k.clust_need && big >= k.blob_need) ? 1 : 0), sys_flags);
    } else {
      if (centres) centres[f] = ncentres;
      if (blobs) blobs[f] = total[1];
      if (largest) largest[f] = big;
      if (box) box[f] = BlobBox{(unsigned short)total[4], (unsigned short)(total[5] + (unsigned int)k.y_lo), (unsigned short)total[6],
                                (unsigned short)(total[7] + (unsigned int)k.y_lo)};
      if (flags) flags[f] = (unsigned char)((ncentres >= k.clust_need && big >= k.blob_need) ? 1 : 0);
    }
  }
}

namespace {

template <int REC, bool PIPE>
hipError_t launch_frames(const BlobLaunch &L) {
  auto kern = blobs_frames_kernel<kBlobBlock, kBlobUnroll, REC, PIPE>;
  static std::atomic<unsigned long long> ready{0ull};
  const WorkItem *work = static_cast<const WorkItem *>(L.plan_ws);
  return launch_over_list(kern, ready, L, L.n_frames, [&](unsigned long long i0, unsigned int n) {
    hipLaunchKernelGGL(kern, dim3(n), dim3(kBlobBlock), L.lds_bytes, L.stream, L.mv, work, (unsigned int)i0, L.n_frames, L.k,
                       L.stream_off, L.n_streams, L.keep, L.flags, L.centres, L.blobs, L.largest, L.box, L.sys_flags, L.sys_centres);
  });
}

}  // namespace

hipError_t launch_blob_scan(const BlobLaunch &L) {
  if (L.n_frames == 0) return hipSuccess;
  if (L.rec_bytes != 40 && L.rec_bytes != 8) return hipErrorInvalidValue;
  if (!L.flags && !L.centres && !L.blobs && !L.largest && !L.box) return hipErrorInvalidValue;
  if (L.pipe) {
    if (L.blobs || (L.centres && L.largest) || ((uintptr_t)L.box & 7u) != 0u) return hipErrorInvalidValue;
  } else {
    if (L.sys_flags != 0 || L.sys_centres != 0) return hipErrorInvalidValue;
    if (L.keep ? (!L.stream_off || L.n_streams == 0) : (L.stream_off != nullptr || L.n_streams != 0)) return hipErrorInvalidValue;
  }
  if (!check_batch_launch(L) || !check_rows(L.k, L.lds_bytes, L.lds_max, blob_lds_bytes(L.k.gw, L.k.R)) ||
      (size_t)L.k.tile_words != blob_tile_words(L.k.gw, L.k.R) || L.k.W != (L.k.gw + 63) / 64)
    return hipErrorInvalidValue;
  // pipe form: the planner's count array is whichever is given; the boxed kernel where the batch has a box array
  return plan_and_launch(
      L, L.pipe, L.flags, L.sys_flags, L.centres ? L.centres : L.largest, L.sys_centres,
      [&](unsigned int grid) {
        hipLaunchKernelGGL(blobs_clear_kernel, dim3(grid), dim3(256), 0, L.stream, L.flags, L.centres, L.blobs, L.largest, L.box,
                           L.n_frames);
      },
      [&](auto rec, auto pipe) {
        if constexpr (pipe()) {
          if (L.box) return launch_frames<rec() | kRecBoxed, true>(L);
        }
        return launch_frames<rec(), pipe()>(L);
      });
}

}  // namespace mtgpu
