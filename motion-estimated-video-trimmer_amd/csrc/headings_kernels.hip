// headings_kernels.hip — object headings: the object scan of objects_kernels.hip and, for each of the K listed blobs of
// a frame, the motion of the records that land in it: a rose of eight sectors, the record count and the summed
// displacement (include/mtgpu_headings.h).  The blobs, their order and the keep mask are the object scan's; "counting
// record", the displacement and the sector are the direction scan's (dir_kernels.hip).  Up to the boxes the kernel IS
// objects_frames_kernel, made of the same shared passes (record_stream.h, blob_label.h, blob_rank.h); what is new
// stands here.
//
//   headings_clear_kernel   fills the non-null outputs ahead of the scan kernel with the answer of a frame without a blob
//                           (0 everywhere, k empty list entries, k empty motion entries): a frame without side data, and
//                           a frame behind the last stream, has no workgroup.
//   headings_frames_kernel  one workgroup per entry of the scan's work list:
//     stream .. boxes   as objects_frames_kernel
//     table       the motion table behind the ranking table is zeroed: per entry 8 bins, a record count, a pad word and
//                 two 64-bit sums (kHeadingTableBytes)
//     ranks       ONE pass over the centre words: the label of every centre becomes the rank of its blob, or kUnlisted.
//                 A centre's root is itself (a root) or its label; the rank is the j with root_of(keys[j]) == root.  A
//                 lane reads and writes its own label only, so the pass needs no barrier inside; the labels are dead
//                 after the boxes.
//     records     the frame's records stream a SECOND time through the unchanged stream_mv40 / stream_compact (the first
//                 pass read them microseconds earlier).  Per record: the bounds and the threshold exactly as vote(); the
//                 centre bit of the destination cell; the rank (one LDS read); then the LDS adds of a belonging record —
//                 its sector's bin (none for a still record), the count, and the two 64-bit sums.
//     store       lane j < k works out `heading` (the largest bin, the lowest sector on a tie) and stores entry j of the
//                 list with one and of the motion with four 16-byte vector stores; a ballot over wave 0 counts the
//                 allowed entries; lane 0 stores the scalars.
//   The no-centre exit is the object scan's plus empty motion entries: a quiet frame reads its records once.
//   Every loop with a barrier inside has a trip count computed from workgroup-uniform values; no loop has an iteration
//   cap.  Every output element has one writer after the clear, plain vector stores, no global atomics.
//
// Three kernels in this unit: the clear and the two record forms (40-byte, 8-byte) of the frames kernel.  There is no
// pipe form.
#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "headings_kernels.hip is written for gfx950 only (wave64, 160 KB LDS)"
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "headings_kernels.h"
#include "record_stream.h"
#include "blob_label.h"
#include "blob_rank.h"

namespace mtgpu {

namespace {

constexpr unsigned int kUnlisted = 0xffffffffu;   // label of a centre whose blob has rank k or beyond

// ranks: the label of every centre -> the rank of its blob among keys[0 .. n), or kUnlisted.  keys[j] holds
// 0xFFFFFFFF - root in its low word (blob_rank::key_of); roots are distinct, so at most one j matches.
template <int BLOCK>
__device__ __forceinline__ void ranks_into_labels(const unsigned long long *cpl, int crows, int W, int gw, unsigned int *L,
                                                  const unsigned long long *keys, int n, int lane) {
  blob_label::for_centre_words<BLOCK>(cpl, crows, W, [&](int r, int w, unsigned long long cw, int tw) {
    if (((cw >> lane) & 1ull) == 0ull) return;
    const unsigned int i = (unsigned int)(r * gw + w * 64 + lane);
    const unsigned int v = L[i];
    const unsigned int p = (v & blob_label::kRoot) ? i : v;
    unsigned int rank = kUnlisted;
    for (int j = 0; j < n; ++j)
      if (0xffffffffu - (unsigned int)(keys[j] & 0xffffffffull) == p) rank = (unsigned int)j;
    L[i] = rank;
  });
}

// ---- one record of the second pass (src/motion_scanner.cpp:246-268 and the sector of include/mtgpu_dir.h): threshold,
// cell and bounds as record_stream.h's vote(); then the centre bit of the destination cell, its rank, and — for a record
// that belongs to a listed blob — the sector as dir_kernels.hip's dir_vote works it out, and the adds.
//   cpl   the centre plane: row r = gy - y_lo < crows, word gx >> 6: inside its crows * W words
//   L     the ranks: word r * gw + gx, inside the crows * gw labels
//   mot   the motion table: entry `rank` < topk at mot + rank * kHeadingTableWords
__device__ __forceinline__ void belong(const MvFields m, const BlobK &k, const unsigned long long *cpl, const unsigned int *L,
                                       unsigned int *mot) {
  const int sdx = m.dst_x - m.src_x, sdy = m.dst_y - m.src_y;  // |.| <= 65535
  const unsigned int dx = (unsigned int)sdx, dy = (unsigned int)sdy;
  // dx*dx < 2^32 exactly; the sum needs 34 bits
  const unsigned long long mag = (unsigned long long)(dx * dx) + (unsigned long long)(dy * dy);
  const int gx = m.dst_x >> k.shift, gy = m.dst_y >> k.shift;
  // 0 <= gx < gw and y_lo <= gy < y_hi (:262) as two unsigned compares (y_hi >= y_lo by construction)
  const bool in = ((unsigned int)gx < (unsigned int)k.gw) & ((unsigned int)(gy - k.y_lo) < (unsigned int)(k.y_hi - k.y_lo));
  if (in & (mag >= k.thr)) {
    const int r = gy - k.y_lo;
    if (((cpl[r * k.W + (gx >> 6)] >> (gx & 63)) & 1ull) != 0ull) {
      const unsigned int rank = L[(unsigned int)(r * k.gw + gx)];
      if (rank != kUnlisted) {
        const unsigned int ax = (unsigned int)(sdx < 0 ? -sdx : sdx), ay = (unsigned int)(sdy < 0 ? -sdy : sdy);
        const bool e = __umul24(12u, ay) <= __umul24(5u, ax), s = __umul24(12u, ax) <= __umul24(5u, ay);
        const unsigned int sx = dx >> 31, sy = dy >> 31;
        const unsigned int diag = 1u | ((sx ^ sy) << 1);
        const unsigned int mid = s ? 2u : diag;
        const unsigned int south = mid | (sy << 2), west = sx << 2;
        const unsigned int sec = e ? west : south;
        unsigned int *ent = mot + rank * (unsigned int)kHeadingTableWords;
        if ((dx | dy) != 0u) atomicAdd(&ent[sec], 1u);
        atomicAdd(&ent[8], 1u);
        atomicAdd(reinterpret_cast<unsigned long long *>(ent + 10), (unsigned long long)(long long)sdx);
        atomicAdd(reinterpret_cast<unsigned long long *>(ent + 12), (unsigned long long)(long long)sdy);
      }
    }
  }
}

// An entry of `motion` without a blob: all zeros, heading = kNoHeading (word 1 of the third vector).
__device__ __forceinline__ void store_empty_heading(ObjectWord4 *o) {
  o[0] = ObjectWord4{0u, 0u, 0u, 0u};
  o[1] = ObjectWord4{0u, 0u, 0u, 0u};
  o[2] = ObjectWord4{0u, kNoHeading, 0u, 0u};
  o[3] = ObjectWord4{0u, 0u, 0u, 0u};
}

}  // namespace

__global__ __launch_bounds__(256) void headings_clear_kernel(unsigned char *__restrict__ flags, unsigned int *__restrict__ centres,
                                                             unsigned int *__restrict__ blobs, unsigned int *__restrict__ objects,
                                                             ObjectWord4 *__restrict__ list, ObjectWord4 *__restrict__ motion,
                                                             unsigned int *__restrict__ allowed, unsigned int n, unsigned int topk) {
  const unsigned long long first = (unsigned long long)blockIdx.x * 256ull + threadIdx.x, step = (unsigned long long)gridDim.x * 256ull;
  for (unsigned long long i = first; i < n; i += step) {
    if (flags) flags[i] = (unsigned char)0;
    if (centres) centres[i] = 0u;
    if (blobs) blobs[i] = 0u;
    if (objects) objects[i] = 0u;
    if (allowed) allowed[i] = 0u;
  }
  const unsigned long long entries = (unsigned long long)n * topk;
  if (list)
    for (unsigned long long i = first; i < entries; i += step) list[i] = ObjectWord4{0u, kNoObjectFirst, kNoObjectBox, kNoObjectBox};
  if (motion)
    for (unsigned long long i = first; i < entries * 4ull; i += step)
      motion[i] = ObjectWord4{0u, (i & 3ull) == 2ull ? kNoHeading : 0u, 0u, 0u};
}

// Waves per SIMD: as objects_frames_kernel — two 1080p workgroups of 16 waves share a CU, eight waves per SIMD and so at
// most 64 VGPRs.  REC: 8 or 40, the bytes per record.  topk: 1 .. kObjectsMax, the entries per frame and the size of the
// ranking table and of the motion table behind `total`.
template <int BLOCK, int UNROLL, int REC>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void headings_frames_kernel(
    const unsigned char *__restrict__ mv, const WorkItem *__restrict__ work, unsigned int item0, unsigned int n_items, BlobK k,
    const unsigned long long *__restrict__ stream_off, unsigned int n_streams, const unsigned long long *__restrict__ keep,
    unsigned char *__restrict__ flags, unsigned int *__restrict__ centres, unsigned int *__restrict__ blobs,
    unsigned int *__restrict__ objects, ObjectWord4 *__restrict__ list, ObjectWord4 *__restrict__ motion,
    unsigned int *__restrict__ allowed, int topk, unsigned int obj_need, unsigned int allow) {
  static_assert(BLOCK % 64 == 0 && kObjectsMax <= 64, "a wave owns one word of the centre plane; lane j of wave 0 stores entry j");
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
  unsigned int *mot = box + 4 * topk;                                               // topk x kHeadingTableWords
  const int t0 = max(k.y_lo - 1, 0), t1 = min(k.y_hi + 1, k.gh);
  const int crows = k.y_hi - k.y_lo;
  const int W = k.W, gw = k.gw;

  // The frame's stream, under a mask only (as objects_frames_kernel): s == n_streams: the frame lies behind the last
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
  ObjectWord4 *mymot = motion ? motion + (size_t)f * (size_t)topk * 4u : nullptr;
  if (ncentres == 0u) {                                       // workgroup-uniform: most frames of most streams
    if (tid == 0) {
      if (centres) centres[f] = 0u;
      if (blobs) blobs[f] = 0u;
      if (objects) objects[f] = 0u;
      if (allowed) allowed[f] = 0u;
      if (flags) flags[f] = (unsigned char)0;
    }
    if (mine && tid < topk) mine[tid] = ObjectWord4{0u, kNoObjectFirst, kNoObjectBox, kNoObjectBox};
    if (mymot && tid < topk) store_empty_heading(mymot + 4 * tid);
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
  // ---- the motion table zeroed (topk * kHeadingTableWords <= 224 words), the labels turned into ranks
  if (tid < topk * kHeadingTableWords) mot[tid] = 0u;
  ranks_into_labels<BLOCK>(cpl, crows, W, gw, L, keys, nblobs, lane);
  __syncthreads();
  // ---- the records again: the belonging ones into the table (crows > 0: there is a centre)
  {
    const auto two = [=, &k](const MvFields m) { belong(m, k, cpl, L, mot); };
    if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(mv + me.r0 * 8ull, me.r1 - me.r0, two);
    else stream_mv40<BLOCK, UNROLL>(mv + me.r0 * 40ull, me.r1 - me.r0, two);
  }
  __syncthreads();
  // ---- store: rows offset by y_lo, `first` by y_lo * gw (a root's index is r * gw + x, r = y - y_lo)
  if (tid >= 64) return;                                      // wave 0: lane j holds entry j
  bool ok = false;
  if (tid < topk) {
    ObjectWord4 e{0u, kNoObjectFirst, kNoObjectBox, kNoObjectBox};
    ObjectWord4 h0{0u, 0u, 0u, 0u}, h1{0u, 0u, 0u, 0u}, h2{0u, kNoHeading, 0u, 0u}, h3{0u, 0u, 0u, 0u};
    if (tid < nblobs) {
      const unsigned long long key = keys[tid];
      const unsigned int *bx = box + 4 * tid;
      e.x = (unsigned int)(key >> 32);
      e.y = 0xffffffffu - (unsigned int)(key & 0xffffffffull) + (unsigned int)(k.y_lo * gw);
      e.z = (bx[0] & 0xffffu) | (((bx[1] + (unsigned int)k.y_lo) & 0xffffu) << 16);
      e.w = (bx[2] & 0xffffu) | (((bx[3] + (unsigned int)k.y_lo) & 0xffffu) << 16);
      const unsigned int *ent = mot + tid * kHeadingTableWords;
      unsigned int best = 0u, head = kNoHeading;              // the largest bin, the lowest sector on a tie
#pragma unroll
      for (unsigned int j = 0; j < 8u; ++j) {
        const unsigned int n = ent[j];
        if (n > best) { best = n; head = j; }
      }
      h0 = ObjectWord4{ent[0], ent[1], ent[2], ent[3]};
      h1 = ObjectWord4{ent[4], ent[5], ent[6], ent[7]};
      h2 = ObjectWord4{ent[8], head, ent[10], ent[11]};
      h3 = ObjectWord4{ent[12], ent[13], 0u, 0u};
      // a still object has no direction to object to
      ok = e.x >= k.blob_need && (head == kNoHeading || ((allow >> head) & 1u) != 0u);
    }
    if (mine) mine[tid] = e;
    if (mymot) {
      ObjectWord4 *o = mymot + 4 * tid;
      o[0] = h0; o[1] = h1; o[2] = h2; o[3] = h3;
    }
  }
  const unsigned int nallowed = (unsigned int)__popcll(__ballot(ok));
  if (tid == 0) {
    if (centres) centres[f] = ncentres;
    if (blobs) blobs[f] = total[1];
    if (objects) objects[f] = total[2];
    if (allowed) allowed[f] = nallowed;
    if (flags) flags[f] = (unsigned char)((ncentres >= k.clust_need && nallowed >= obj_need) ? 1 : 0);
  }
}

namespace {

template <int REC>
hipError_t launch_frames(const HeadLaunch &L) {
  auto kern = headings_frames_kernel<kHeadingsBlock, kHeadingsUnroll, REC>;
  static std::atomic<unsigned long long> ready{0ull};
  const WorkItem *work = static_cast<const WorkItem *>(L.plan_ws);
  return launch_over_list(kern, ready, L, L.n_frames, [&](unsigned long long i0, unsigned int n) {
    hipLaunchKernelGGL(kern, dim3(n), dim3(kHeadingsBlock), L.lds_bytes, L.stream, L.mv, work, (unsigned int)i0, L.n_frames, L.k,
                       L.stream_off, L.n_streams, L.keep, L.flags, L.centres, L.blobs, L.objects, L.list, L.motion, L.allowed,
                       L.topk, L.obj_need, L.allow);
  });
}

}  // namespace

hipError_t launch_heading_scan(const HeadLaunch &L) {
  if (L.n_frames == 0) return hipSuccess;
  if (L.rec_bytes != 40 && L.rec_bytes != 8) return hipErrorInvalidValue;
  if (L.topk < 1 || L.topk > kObjectsMax || ((uintptr_t)L.list & 15u) != 0u || ((uintptr_t)L.motion & 15u) != 0u) return hipErrorInvalidValue;
  if (L.allow > 255u || L.obj_need < 1u || L.obj_need > (unsigned int)L.topk) return hipErrorInvalidValue;
  if (!L.flags && !L.centres && !L.blobs && !L.objects && !L.list && !L.motion && !L.allowed) return hipErrorInvalidValue;
  if (L.keep ? (!L.stream_off || L.n_streams == 0) : (L.stream_off != nullptr || L.n_streams != 0)) return hipErrorInvalidValue;
  if (!check_batch_launch(L) || !check_rows(L.k, L.lds_bytes, L.lds_max, headings_lds_bytes(L.k.gw, L.k.R, L.topk)) ||
      (size_t)L.k.tile_words != blob_tile_words(L.k.gw, L.k.R) || L.k.W != (L.k.gw + 63) / 64)
    return hipErrorInvalidValue;
  return plan_and_launch(
      L, false, nullptr, 0, nullptr, 0,
      [&](unsigned int grid) {
        hipLaunchKernelGGL(headings_clear_kernel, dim3(grid), dim3(256), 0, L.stream, L.flags, L.centres, L.blobs, L.objects, L.list,
                           L.motion, L.allowed, L.n_frames, (unsigned int)L.topk);
      },
      [&](auto rec, auto) { return launch_frames<rec()>(L); });
}

}  // namespace mtgpu
