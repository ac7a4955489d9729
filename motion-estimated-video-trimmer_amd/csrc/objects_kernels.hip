// objects_kernels.hip — object lists: the K largest blobs of every frame, ranked and boxed, and the number of blobs of a
// minimum size (include/mtgpu_objects.h).  The blobs are those of blobs_kernels.hip — the 4-connected components of the
// centre cells of src/motion_scanner.cpp:272-294, with or without a keep mask — and up to the labels the kernel IS
// blobs_frames_kernel's resident form; what is new stands in blob_rank.h.
//
//   objects_clear_kernel    fills the non-null outputs ahead of the scan kernel with the answer of a frame without a blob
//                           (0 everywhere, k empty entries): a frame without side data, and a frame behind the last
//                           stream, has no workgroup.
//   objects_frames_kernel   one workgroup per entry of the scan's work list:
//     stream, keep, votes, masks, centres, no centre     as blobs_frames_kernel (record_stream.h)
//     labels      blob_label::init, unite_rows, flatten, a barrier behind each: a root holds kRoot | (cells - 1) and is
//                 the smallest cell index of its blob, every other centre holds its root
//     count       over the roots: the blobs, and the blobs of at least blob_need cells — over ALL blobs, listed or not;
//                 inside round 0 of the ranking, which meets every root anyway
//     rank        rounds of a 64-bit LDS atomicMax on the winner key cells << 32 | (0xFFFFFFFF - root); round j admits
//                 the keys strictly below round j - 1's.  min(k, blobs) rounds: the blob count is an LDS word read
//                 behind round 0's barrier, so the trip count is workgroup-uniform, and a frame with one blob — most
//                 frames that have any — runs one round.  Keys are distinct: the order does not depend on timing.
//     boxes       ONE pass over the centre words for all listed blobs: a cell's key against the least listed key, then
//                 min / max of the four bounds per (wave, distinct listed root)
//     store       lane j < k stores entry j with one 16-byte vector store, lane 0 the scalars
//   Every loop with a barrier inside has a trip count computed from workgroup-uniform values; no loop has an iteration
//   cap.  Every output element has one writer after the clear, plain vector stores, no global atomics.
//
// Three kernels in this unit: the clear and the two record forms (40-byte, 8-byte) of the frames kernel.  There is no
// pipe form.
#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "objects_kernels.hip is written for gfx950 only (wave64, 160 KB LDS)"
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "objects_kernels.h"
#include "record_stream.h"
#include "blob_label.h"
#include "blob_rank.h"

namespace mtgpu {

__global__ __launch_bounds__(256) void objects_clear_kernel(unsigned char *__restrict__ flags, unsigned int *__restrict__ centres,
                                                            unsigned int *__restrict__ blobs, unsigned int *__restrict__ objects,
                                                            ObjectWord4 *__restrict__ list, unsigned int n, unsigned int topk) {
  const unsigned long long first = (unsigned long long)blockIdx.x * 256ull + threadIdx.x, step = (unsigned long long)gridDim.x * 256ull;
  for (unsigned long long i = first; i < n; i += step) {
    if (flags) flags[i] = (unsigned char)0;
    if (centres) centres[i] = 0u;
    if (blobs) blobs[i] = 0u;
    if (objects) objects[i] = 0u;
  }
  if (list) {
    const unsigned long long entries = (unsigned long long)n * topk;
    for (unsigned long long i = first; i < entries; i += step) list[i] = ObjectWord4{0u, kNoObjectFirst, kNoObjectBox, kNoObjectBox};
  }
}

// Waves per SIMD: as blobs_frames_kernel — two 1080p workgroups of 16 waves share a CU, eight waves per SIMD and so at
// most 64 VGPRs.  REC: 8 or 40, the bytes per record.  topk: 1 .. kObjectsMax, the entries per frame and the size of the
// ranking table behind `total`.
template <int BLOCK, int UNROLL, int REC>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void objects_frames_kernel(
    const unsigned char *__restrict__ mv, const WorkItem *__restrict__ work, unsigned int item0, unsigned int n_items, BlobK k,
    const unsigned long long *__restrict__ stream_off, unsigned int n_streams, const unsigned long long *__restrict__ keep,
    unsigned char *__restrict__ flags, unsigned int *__restrict__ centres, unsigned int *__restrict__ blobs,
    unsigned int *__restrict__ objects, ObjectWord4 *__restrict__ list, int topk, unsigned int obj_need) {
  static_assert(BLOCK % 64 == 0 && BLOCK >= kObjectsMax, "a wave owns one word of the centre plane; lane j stores entry j");
  static_assert(REC == 8 || REC == 40, "8 or 40 bytes per record");
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
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(total + 8);     // topk keys
  unsigned int *box = reinterpret_cast<unsigned int *>(keys + topk);                // topk x 4 bounds
  const int t0 = max(k.y_lo - 1, 0), t1 = min(k.y_hi + 1, k.gh);
  const int crows = k.y_hi - k.y_lo;
  const int W = k.W, gw = k.gw;

  // The frame's stream, under a mask only (as blobs_frames_kernel): s == n_streams: the frame lies behind the last
  // stream and keeps what the clear wrote.
  const unsigned int f = __builtin_amdgcn_readfirstlane(me.f);
  const bool masked = keep != nullptr;
  unsigned int s = 0u;
  if (masked) {
    s = stream_of(stream_off, n_streams, f);
    if (s >= n_streams) return;
  }

  // ---- the keep words of the analysed rows (no mask: ones), the first word of a lane on its way while the tile is zeroed
  const int nkeep = crows * W;
  const unsigned long long *kp = masked ? keep + ((size_t)s * (size_t)k.gh + (size_t)k.y_lo) * (size_t)W : nullptr;
  const unsigned long long k0 = (masked && tid < nkeep) ? kp[tid] : ~0ull;
  zero_tile<BLOCK>(tile, k.tile_words);
  if (tid < 8) total[tid] = 0u;
  if (tid < topk) {                                            // the ranking table: no key, empty boxes
    keys[tid] = 0ull;
    box[4 * tid + 0] = 0xffffffffu; box[4 * tid + 1] = 0xffffffffu; box[4 * tid + 2] = 0u; box[4 * tid + 3] = 0u;
  }
  if (tid < nkeep) klds[tid] = k0;
  for (int j = tid + BLOCK; j < nkeep; j += BLOCK) klds[j] = masked ? kp[j] : ~0ull;
  __syncthreads();
  // ---- the votes (an empty analysed range keeps nothing: nothing to read)
  if (crows > 0) {
    const auto one = [=, &k](const MvFields m) { vote(m, k, t0, tile); };
    if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(mv + me.r0 * 8ull, me.r1 - me.r0, one);
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
  ObjectWord4 *mine = list ? list + (size_t)f * (size_t)topk : nullptr;
  if (ncentres == 0u) {                                       // workgroup-uniform: most frames of most streams
    if (tid == 0) {
      if (centres) centres[f] = 0u;
      if (blobs) blobs[f] = 0u;
      if (objects) objects[f] = 0u;
      if (flags) flags[f] = (unsigned char)0;
    }
    if (mine && tid < topk) mine[tid] = ObjectWord4{0u, kNoObjectFirst, kNoObjectBox, kNoObjectBox};
    return;
  }

  // ---- labels.  L[r * gw + x], r < crows <= R: inside the tile's (R + 2) * gw words.
  unsigned int *L = tile;
  blob_label::init<BLOCK>(cpl, crows, W, gw, L, lane);
  __syncthreads();
  blob_label::unite_rows<BLOCK>(cpl, crows, W, gw, L, lane);
  __syncthreads();
  blob_label::flatten<BLOCK>(cpl, crows, W, gw, L, lane);
  __syncthreads();
  // ---- round 0 meets every root: it also counts them
  blob_rank::rank_round<BLOCK, true>(cpl, crows, W, gw, L, &keys[0], ~0ull, total, k.blob_need, lane);
  __syncthreads();
  const int nblobs = (int)min(total[1], (unsigned int)topk);  // >= 1: there is a centre.  The listed blobs, and the rounds
  for (int j = 1; j < nblobs; ++j) {                          // workgroup-uniform trip count
    blob_rank::rank_round<BLOCK, false>(cpl, crows, W, gw, L, &keys[j], keys[j - 1], total, k.blob_need, lane);
    __syncthreads();
  }
  blob_rank::boxes<BLOCK>(cpl, crows, W, gw, L, keys, box, nblobs, lane);
  __syncthreads();
  // ---- store: rows offset by y_lo, `first` by y_lo * gw (a root's index is r * gw + x, r = y - y_lo)
  if (mine && tid < topk) {
    ObjectWord4 e{0u, kNoObjectFirst, kNoObjectBox, kNoObjectBox};
    if (tid < nblobs) {
      const unsigned long long key = keys[tid];
      const unsigned int *bx = box + 4 * tid;
      e.x = (unsigned int)(key >> 32);
      e.y = 0xffffffffu - (unsigned int)(key & 0xffffffffull) + (unsigned int)(k.y_lo * gw);
      e.z = (bx[0] & 0xffffu) | (((bx[1] + (unsigned int)k.y_lo) & 0xffffu) << 16);
      e.w = (bx[2] & 0xffffu) | (((bx[3] + (unsigned int)k.y_lo) & 0xffffu) << 16);
    }
    mine[tid] = e;
  }
  if (tid == 0) {
    const unsigned int nobj = total[2];
    if (centres) centres[f] = ncentres;
    if (blobs) blobs[f] = total[1];
    if (objects) objects[f] = nobj;
    if (flags) flags[f] = (unsigned char)((ncentres >= k.clust_need && nobj >= obj_need) ? 1 : 0);
  }
}

namespace {

template <int REC>
hipError_t launch_frames(const ObjLaunch &L) {
  auto kern = objects_frames_kernel<kObjectsBlock, kObjectsUnroll, REC>;
  static std::atomic<unsigned long long> ready{0ull};
  const WorkItem *work = static_cast<const WorkItem *>(L.plan_ws);
  return launch_over_list(kern, ready, L, L.n_frames, [&](unsigned long long i0, unsigned int n) {
    hipLaunchKernelGGL(kern, dim3(n), dim3(kObjectsBlock), L.lds_bytes, L.stream, L.mv, work, (unsigned int)i0, L.n_frames, L.k,
                       L.stream_off, L.n_streams, L.keep, L.flags, L.centres, L.blobs, L.objects, L.list, L.topk, L.obj_need);
  });
}

}  // namespace

hipError_t launch_object_scan(const ObjLaunch &L) {
  if (L.n_frames == 0) return hipSuccess;
  if (L.rec_bytes != 40 && L.rec_bytes != 8) return hipErrorInvalidValue;
  if (L.topk < 1 || L.topk > kObjectsMax || ((uintptr_t)L.list & 15u) != 0u) return hipErrorInvalidValue;
  if (!L.flags && !L.centres && !L.blobs && !L.objects && !L.list) return hipErrorInvalidValue;
  if (L.keep ? (!L.stream_off || L.n_streams == 0) : (L.stream_off != nullptr || L.n_streams != 0)) return hipErrorInvalidValue;
  if (!check_batch_launch(L) || !check_rows(L.k, L.lds_bytes, L.lds_max, objects_lds_bytes(L.k.gw, L.k.R, L.topk)) ||
      (size_t)L.k.tile_words != blob_tile_words(L.k.gw, L.k.R) || L.k.W != (L.k.gw + 63) / 64)
    return hipErrorInvalidValue;
  return plan_and_launch(
      L, false, nullptr, 0, nullptr, 0,
      [&](unsigned int grid) {
        hipLaunchKernelGGL(objects_clear_kernel, dim3(grid), dim3(256), 0, L.stream, L.flags, L.centres, L.blobs, L.objects, L.list,
                           L.n_frames, (unsigned int)L.topk);
      },
      [&](auto rec, auto) { return launch_frames<rec()>(L); });
}

}  // namespace mtgpu
