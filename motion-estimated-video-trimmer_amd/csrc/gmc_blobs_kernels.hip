// gmc_blobs_kernels.hip — the compensated blob scan: motion blobs on the residuals of every frame's dominant vector
// (include/mtgpu_gmc_blobs.h).  The estimate is that of gmc_kernels.hip (under a keep mask, the masked estimate of its
// pipe form), the active plane that of zones_kernels.hip, the labelling that of blobs_kernels.hip; what is new is that
// the residual vote, which lives only in a workgroup's LDS tile, is labelled before the workgroup ends.  Two forms: the
// resident one and the pipe form of include/mtgpu_pipe_gmc_blobs.h, the decode path's third mode (its two single
// setters, mtgpu_pipe_set_gmc and mtgpu_pipe_set_blobs, still refuse each other).
//
//   gmc_blobs_clear_kernel    fills the non-null outputs ahead of the scan kernel with the answer of a frame without a
//                             blob (0 everywhere, an all-0xFFFF box, a zero info): a frame without side data, and a
//                             frame behind the last stream, has no workgroup.
//   gmc_blobs_frames_kernel   one workgroup per entry of the scan's work list:
//     stream, keep   as blobs_frames_kernel: under a mask the frame's stream by binary search (a frame behind the last
//                    stream returns before any barrier) and its keep words of the analysed rows into LDS; no mask: ones,
//                    no stream lookup.
//     estimate    hist_add per axis for every counted record — inside the bounds of :262 and, under a mask, with the
//                 keep bit of its destination cell set: one LDS read of the staged keep word per record inside the
//                 bounds, behind the workgroup-uniform `masked` branch; the unmasked path streams with the functor of
//                 gmc_frames_kernel.
//     pick        wave 0, pick_mode per axis and the support test, as gmc_frames_kernel.
//     vote        the same records a second time, on the residuals, squares in 64 bits.
//     masks       row_masks ANDed with the staged keep rows (halo rows unmasked), as blobs_frames_kernel.
//     centres     centre_word of every (analysed row, word) into the centre plane, over the keep words — dead by then —
//                 and the count.
//     no centre   a workgroup-uniform test: lane 0 stores the zeros AND the info, and the workgroup ends.
//     labels      the five passes of blob_label.h over the dead vote tile: init, unite, flatten, winner, box.
//   Every loop with a barrier inside has a trip count computed from workgroup-uniform values; no barrier sits inside a
//   non-uniform branch.  Every output element has one writer after the clear: lane 0 of the frame's workgroup, plain
//   vector stores, no global atomics.  The planner answers nothing itself (the outputs hold the clear's values).
//
// The pipe form (PIPE, include/mtgpu_pipe_gmc_blobs.h) follows the cut of gmc_frames_kernel and blobs_frames_kernel: no
// clear kernel — the planner answers the frames without side data at the outputs' scope; no stream lookup — `keep` is ONE
// plane of gh x W words or null, staged into the same keep rows; BOTH exits store the flag and ONE count (centres, the
// largest blob, or the applied vector, by `report`) through store_flag / store_centres, because a reused pinned block
// holds the previous batch's values; no box pass, no blobs, no info — except in the boxed pipe form (REC | kRecBoxed;
// MT_LAYOUT_BOXES, include/mtgpu_pipe_boxes.h), which runs the box pass and its barrier on the final exit and stores the
// winner's box with one 8-byte store at the flags' scope.  The flag pointer, the count pointer, the scopes and
// the report are re-taken from the kernel-argument segment where they are used, as `out` is in the resident form.
//
// record_stream.h is used as it is; walk_value and pick_mode are those of gmc_kernels.hip, restated here because that
// file stays as it is and keeps them in its unnamed namespace; hist_add makes the same adds with one branch less.
#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "gmc_blobs_kernels.hip is written for gfx950 only (wave64, 160 KB LDS)"
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "gmc_blobs_kernels.h"
#include "record_stream.h"
#include "blob_label.h"

namespace mtgpu {

namespace {

// One add into bin `bin` of `h` for every lane with `on`: the lanes whose bin equals the first active lane's are added
// by that lane in one atomic; the others add for themselves (a pan puts a wave's 64 records into ONE bin per axis).
__device__ __forceinline__ void hist_add(unsigned int *h, int bin, bool on) {
  if (!on) return;
  const int lead = __builtin_amdgcn_readfirstlane(bin);       // the first active lane's bin
  const bool same = bin == lead;
  const unsigned long long grp = __ballot(same);              // among the active lanes; the first one is in it
  const bool leader = same && (int)__lane_id() == __ffsll((long long)grp) - 1;
  // one atomic under one mask: the leader adds its group, a lane that disagrees adds for itself
  if (leader || !same) atomicAdd(&h[bin], leader ? (unsigned int)__popcll(grp) : 1u);
}

// Walk index o in [0, 2 * max_shift] -> candidate: 0, -1, +1, -2, +2, ...
__device__ __forceinline__ int walk_value(int o) { return (o & 1) ? -((o + 1) >> 1) : (o >> 1); }

// The mode of one axis: (count << 8 | 255 - o) of the winning candidate, on every lane of wave 0.
__device__ __forceinline__ unsigned long long pick_mode(const unsigned int *h, int ms, int lane) {
  unsigned long long best = 0ull;
  for (int o = lane; o <= 2 * ms; o += 64) {
    const unsigned long long key = ((unsigned long long)h[walk_value(o) + ms] << 8) | (unsigned long long)(255 - o);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long other = __shfl_xor(best, d);
    best = other > best ? other : best;
  }
  return best;
}

// mt_gmc_info of frame f from the estimate's result words: int16 gx, gy, mode_x, mode_y; u32 n_in, n_x, n_y
__device__ __forceinline__ void store_info(unsigned int *info, unsigned int f, const unsigned int *res) {
  unsigned int *o = info + (unsigned long long)f * kGmcInfoWords;
  o[0] = (res[2] & 0xffffu) | (res[3] << 16);
  o[1] = (res[4] & 0xffffu) | (res[5] << 16);
  o[2] = res[1];
  o[3] = res[6];
  o[4] = res[7];
}

// The launch's argument block where the kernel finds it: at the start of the kernel-argument segment (constant memory).
typedef const __attribute__((address_space(4))) GmcBlobArgs *LateArgs;

// The six output pointers, loaded here and now (member by member: scalar loads from the argument segment).
__device__ __forceinline__ GmcBlobOut late_outputs(LateArgs late) {
  GmcBlobOut o;
  o.flags = late->out.flags;
  o.centres = late->out.centres;
  o.blobs = late->out.blobs;
  o.largest = late->out.largest;
  o.box = late->out.box;
  o.info = late->out.info;
  return o;
}

// The pipe form's count of a frame: its centres, its largest blob, or the applied vector of the estimate in `res`.
__device__ __forceinline__ unsigned int pipe_count(int report, unsigned int ncentres, unsigned int big, const unsigned int *res) {
  return report == kGmcBlobReportVector ? ((res[2] & 0xffffu) | (res[3] << 16)) : report == kGmcBlobReportLargest ? big : ncentres;
}

}  // namespace

__global__ __launch_bounds__(256) void gmc_blobs_clear_kernel(unsigned char *__restrict__ flags, unsigned int *__restrict__ centres,
                                                              unsigned int *__restrict__ blobs, unsigned int *__restrict__ largest,
                                                              BlobBox *__restrict__ box, unsigned int *__restrict__ info,
                                                              unsigned int n) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull) {
    if (flags) flags[i] = (unsigned char)0;
    if (centres) centres[i] = 0u;
    if (blobs) blobs[i] = 0u;
    if (largest) largest[i] = 0u;
    if (box) box[i] = BlobBox{0xffffu, 0xffffu, 0xffffu, 0xffffu};
    if (info) {
#pragma unroll
      for (int j = 0; j < kGmcInfoWords; ++j) info[i * (unsigned long long)kGmcInfoWords + j] = 0u;
    }
  }
}

// Waves per SIMD as the parents: a 1080p workgroup takes 34 848 bytes of LDS, two workgroups of 16 waves share a CU, eight
// waves per SIMD and so at most 64 VGPRs; the 4K workgroup sits alone on its CU.
// PIPE: the form for a pipe's staging batch — stream_off / n_streams are not read (null / 0), `keep` is ONE plane (gh x W
// words) or null, of `out` only flags and centres are read — centres is the batch's ONE count array, whatever it
// carries — and the results leave through store_flag / store_centres with sys_flags / sys_count.  !PIPE: sys_* and
// report are not read (0).
// REC: 8 or 40, the bytes per record; | kRecBoxed (blobs_kernels.h): the boxed pipe form (MT_LAYOUT_BOXES,
// include/mtgpu_pipe_boxes.h) — out.box is the batch's box array, 8-byte aligned; the final exit runs the box pass and its
// barrier and stores the winner's box.  The early exit and the planner store no box: it is specified only where the flag
// is set.
template <int BLOCK, int UNROLL, int REC, bool PIPE>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void gmc_blobs_frames_kernel(const GmcBlobArgs a) {
  static_assert(BLOCK % 64 == 0, "a wave owns one word of the centre plane");
  static_assert(BLOCK >= 2 * kGmcHistBins + 16, "one lane per word of hist, res and total");
  constexpr bool BOXED = (REC & kRecBoxed) != 0;     // the boxed pipe form: out.box is the batch's box array
  constexpr int RB = REC & ~kRecBoxed;               // bytes per record
  static_assert((RB == 8 || RB == 40) && (PIPE || !BOXED), "8 or 40 bytes per record; the boxed form is a pipe form");
  extern __shared__ __attribute__((aligned(16))) unsigned int lds[];
  const unsigned int item = a.item0 + blockIdx.x;
  if (item >= a.n_items) return;
  const WorkItem me = load_item(a.work, item);
  if (me.f == kNoFrame) return;                 // the list has ended (every later entry is past its end too)
  const GmcBlobK &k = a.k;
  const unsigned char *mv = a.mv;
  const unsigned long long *stream_off = a.stream_off, *keep = a.keep;
  const unsigned int n_streams = a.n_streams;
  // The six output pointers are not read before the workgroup's last lines.  Read from `a` they are loaded with the
  // other arguments at the kernel's entry and held in 12 SGPRs across both record passes, which the compact form's
  // unrolled estimate has no room for (14 SGPR spills to VGPR lanes, measured).  So they are re-taken where they are
  // used, as the pipe form of gmc_frames_kernel re-takes its uniform test: the argument block is the kernel's one
  // argument, so it starts the kernel-argument segment, and `late` reads it there.  Nothing else names a.out.
  const LateArgs late = (LateArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  unsigned int *tile = lds;
  unsigned long long *klds = reinterpret_cast<unsigned long long *>(lds + k.tile_words);
  unsigned long long *amask = klds + (size_t)k.R * k.W;
  unsigned int *hx = reinterpret_cast<unsigned int *>(amask + (size_t)(k.R + 2) * k.W);
  unsigned int *hy = hx + kGmcHistBins;
  unsigned int *res = hy + kGmcHistBins;
  unsigned int *total = res + 8;
  const int t0 = max(k.y_lo - 1, 0), t1 = min(k.y_hi + 1, k.gh);
  const int crows = k.y_hi - k.y_lo;
  const int W = k.W, gw = k.gw;
  const int ms = k.max_shift;
  const unsigned char *recs = mv + me.r0 * (unsigned long long)RB;
  const unsigned long long nrec = me.r1 - me.r0;

  // The frame's stream, under a mask only: s = the number of streams that end at or before frame f (binary search on
  // workgroup-uniform values).  s == n_streams: the frame lies behind the last stream and keeps what the clear wrote.
  const unsigned int f = __builtin_amdgcn_readfirstlane(me.f);
  const bool masked = keep != nullptr;
  unsigned int s = 0u;
  if (!PIPE && masked) {                        // pipe form: plane 0 serves every frame of the batch
    s = stream_of(stream_off, n_streams, f);
    if (s >= n_streams) return;                 // a frame in front of the first stream is not told apart: it takes plane 0
  }

  // ---- the keep words of the analysed rows (no mask: ones; keep row y_lo + r, r < crows, lies inside the stream's
  // gh x W plane), the first word of a lane on its way while the tile, the histograms and the result words are zeroed
  const int nkeep = crows * W;
  const unsigned long long *kp = masked ? keep + ((size_t)s * (size_t)k.gh + (size_t)k.y_lo) * (size_t)W : nullptr;
  const unsigned long long k0 = (masked && tid < nkeep) ? kp[tid] : ~0ull;
  zero_tile<BLOCK>(tile, k.tile_words);
  // hx, hy, res and total are contiguous; total[4], total[5]: minima
  if (tid < 2 * kGmcHistBins + 16) hx[tid] = (tid == 2 * kGmcHistBins + 12 || tid == 2 * kGmcHistBins + 13) ? 0xffffffffu : 0u;
  if (tid < nkeep) klds[tid] = k0;
  for (int j = tid + BLOCK; j < nkeep; j += BLOCK) klds[j] = masked ? kp[j] : ~0ull;
  __syncthreads();
  // ---- the estimate (an empty analysed range counts nothing: nothing to read)
  if (crows > 0) {
    unsigned int mine = 0u;
    if (masked) {
      // counted: inside the bounds AND the keep bit of the destination cell (one LDS read per record inside the bounds;
      // gy - y_lo < crows <= R and gx >> 6 < W: inside the staged rows)
      const auto onek = [=, &k, &mine](const MvFields m) {
        const int gx = m.dst_x >> k.shift, gy = m.dst_y >> k.shift;
        bool in = ((unsigned int)gx < (unsigned int)k.gw) & ((unsigned int)(gy - k.y_lo) < (unsigned int)(k.y_hi - k.y_lo));
        if (in) in = ((klds[(gy - k.y_lo) * k.W + (gx >> 6)] >> (gx & 63)) & 1ull) != 0ull;
        const int dx = m.dst_x - m.src_x, dy = m.dst_y - m.src_y;
        mine += in ? 1u : 0u;
        hist_add(hx, dx + ms, in && (unsigned int)(dx + ms) <= (unsigned int)(2 * ms));
        hist_add(hy, dy + ms, in && (unsigned int)(dy + ms) <= (unsigned int)(2 * ms));
      };
      if constexpr (RB == 8) stream_compact<BLOCK, UNROLL>(recs, nrec, onek);
      else stream_mv40<BLOCK, UNROLL>(recs, nrec, onek);
    } else {
      const auto one = [=, &k, &mine](const MvFields m) {
        const int gx = m.dst_x >> k.shift, gy = m.dst_y >> k.shift;
        const bool in = ((unsigned int)gx < (unsigned int)k.gw) & ((unsigned int)(gy - k.y_lo) < (unsigned int)(k.y_hi - k.y_lo));
        const int dx = m.dst_x - m.src_x, dy = m.dst_y - m.src_y;
        mine += in ? 1u : 0u;
        // |d| <= max_shift as one unsigned compare
        hist_add(hx, dx + ms, in && (unsigned int)(dx + ms) <= (unsigned int)(2 * ms));
        hist_add(hy, dy + ms, in && (unsigned int)(dy + ms) <= (unsigned int)(2 * ms));
      };
      if constexpr (RB == 8) stream_compact<BLOCK, UNROLL>(recs, nrec, one);
      else stream_mv40<BLOCK, UNROLL>(recs, nrec, one);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
    if (lane == 0 && mine) atomicAdd(&res[1], mine);
  }
  __syncthreads();
  // ---- the pick: mode and support of both axes
  if (tid < 64) {
    const unsigned long long bx = pick_mode(hx, ms, tid), by = pick_mode(hy, ms, tid);
    if (tid == 0) {
      const unsigned long long n_in = res[1];
      const unsigned int nx = (unsigned int)(bx >> 8), ny = (unsigned int)(by >> 8);
      const int mx = walk_value(255 - (int)(bx & 255ull)), my = walk_value(255 - (int)(by & 255ull));
      const unsigned long long need = (unsigned long long)k.min_share_q8 * n_in;
      res[2] = (unsigned int)(((unsigned long long)nx << 8) >= need ? mx : 0);
      res[3] = (unsigned int)(((unsigned long long)ny << 8) >= need ? my : 0);
      res[4] = (unsigned int)mx; res[5] = (unsigned int)my;
      res[6] = nx; res[7] = ny;
    }
  }
  __syncthreads();
  const int cgx = __builtin_amdgcn_readfirstlane((int)res[2]), cgy = __builtin_amdgcn_readfirstlane((int)res[3]);
  // ---- the votes on the residuals.  The test is taken anew, as in the pipe form of gmc_frames_kernel (else its result is
  // held across the estimate)
  if (__builtin_amdgcn_readfirstlane(crows) > 0) {
    const auto one = [=, &k](const MvFields m) {
      const int rx = (m.dst_x - m.src_x) - cgx, ry = (m.dst_y - m.src_y) - cgy;   // |r| <= 65535 + 127
      const unsigned int ax = (unsigned int)(rx < 0 ? -rx : rx), ay = (unsigned int)(ry < 0 ? -ry : ry);
      // a square can exceed 2^32: 64-bit products
      const unsigned long long mag = (unsigned long long)ax * ax + (unsigned long long)ay * ay;
      const int gx = m.dst_x >> k.shift, gy = m.dst_y >> k.shift;
      const bool in = ((unsigned int)gx < (unsigned int)k.gw) & ((unsigned int)(gy - k.y_lo) < (unsigned int)(k.y_hi - k.y_lo));
      // gy in [y_lo, y_hi) and t0 <= y_lo: the index stays inside the tile
      if (in && mag >= k.thr) atomicAdd(&tile[(unsigned int)((gy - t0) * k.gw + gx)], 1u);
    };
    if constexpr (RB == 8) stream_compact<BLOCK, UNROLL>(recs, nrec, one);
    else stream_mv40<BLOCK, UNROLL>(recs, nrec, one);
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
    if constexpr (PIPE) {                                     // a reused pinned block holds the previous batch's values
      if (tid == 0) {
        unsigned char *const fl = late->out.flags;
        unsigned int *const cnt = late->out.centres;
        if (cnt) store_centres(cnt, f, pipe_count(late->report, 0u, 0u, res), late->sys_count);
        if (fl) store_flag(fl, f, (unsigned char)0, late->sys_flags);
      }
      return;
    }
    if (tid == 0) {
      const GmcBlobOut o = late_outputs(late);
      if (o.centres) o.centres[f] = 0u;
      if (o.blobs) o.blobs[f] = 0u;
      if (o.largest) o.largest[f] = 0u;
      if (o.box) o.box[f] = BlobBox{0xffffu, 0xffffu, 0xffffu, 0xffffu};
      if (o.flags) o.flags[f] = (unsigned char)0;
      if (o.info) store_info(o.info, f, res);
    }
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
  blob_label::winner<BLOCK>(cpl, crows, W, gw, L, total, lane);
  __syncthreads();
  const unsigned long long key = *reinterpret_cast<const unsigned long long *>(total + 2);
  if constexpr (PIPE && BOXED) {                              // the boxed pipe form: the box pass, then the three stores
    blob_label::box<BLOCK>(cpl, crows, W, gw, L, total, 0xffffffffu - (unsigned int)(key & 0xffffffffull), lane);
    __syncthreads();
    if (tid == 0) {
      const unsigned int big = (unsigned int)(key >> 32);
      unsigned char *const fl = late->out.flags;
      unsigned int *const cnt = late->out.centres;
      BlobBox *const bx = late->out.box;
      if (cnt) store_centres(cnt, f, pipe_count(late->report, ncentres, big, res), late->sys_count);
      // ONE 8-byte store, at the flags' scope: the box array lives in the same block
      store_result(reinterpret_cast<unsigned long long *>(bx) + f, pack_box(total[4], total[5] + (unsigned int)k.y_lo, total[6],
                                                                              total[7] + (unsigned int)k.y_lo), late->sys_flags);
      if (fl) store_flag(fl, f, (unsigned char)((ncentres >= k.clust_need && big >= k.blob_need) ? 1 : 0), late->sys_flags);
    }
    return;
  } else if constexpr (PIPE) {                                // the box serves no output of this form: no pass, no barrier
    if (tid == 0) {
      const unsigned int big = (unsigned int)(key >> 32);
      unsigned char *const fl = late->out.flags;
      unsigned int *const cnt = late->out.centres;
      if (cnt) store_centres(cnt, f, pipe_count(late->report, ncentres, big, res), late->sys_count);
      if (fl) store_flag(fl, f, (unsigned char)((ncentres >= k.clust_need && big >= k.blob_need) ? 1 : 0), late->sys_flags);
    }
    return;
  }
  const unsigned int win = 0xffffffffu - (unsigned int)(key & 0xffffffffull);
  blob_label::box<BLOCK>(cpl, crows, W, gw, L, total, win, lane);
  __syncthreads();
  if (tid == 0) {
    const unsigned int big = (unsigned int)(key >> 32);
    const GmcBlobOut o = late_outputs(late);
    if (o.centres) o.centres[f] = ncentres;
    if (o.blobs) o.blobs[f] = total[1];
    if (o.largest) o.largest[f] = big;
    if (o.box) o.box[f] = BlobBox{(unsigned short)total[4], (unsigned short)(total[5] + (unsigned int)k.y_lo), (unsigned short)total[6],
                                  (unsigned short)(total[7] + (unsigned int)k.y_lo)};
    if (o.flags) o.flags[f] = (unsigned char)((ncentres >= k.clust_need && big >= k.blob_need) ? 1 : 0);
    if (o.info) store_info(o.info, f, res);
  }
}

namespace {

template <int REC, bool PIPE>
hipError_t launch_frames(const GmcBlobLaunch &L) {
  auto kern = gmc_blobs_frames_kernel<kGmcBlobBlock, kGmcBlobUnroll, REC, PIPE>;
  static std::atomic<unsigned long long> ready{0ull};
  GmcBlobArgs a;
  a.mv = L.mv;
  a.work = static_cast<const WorkItem *>(L.plan_ws);
  a.item0 = 0u;
  a.n_items = L.n_frames;
  a.k = L.k;
  a.stream_off = L.stream_off;
  a.n_streams = L.n_streams;
  a.keep = L.keep;
  a.out = GmcBlobOut{L.flags, L.centres, L.blobs, L.largest, L.box, L.info};
  a.sys_flags = L.sys_flags;
  a.sys_count = L.sys_count;
  a.report = L.report;
  return launch_over_list(kern, ready, L, L.n_frames, [&](unsigned long long i0, unsigned int n) {
    a.item0 = (unsigned int)i0;
    hipLaunchKernelGGL(kern, dim3(n), dim3(kGmcBlobBlock), L.lds_bytes, L.stream, a);
  });
}

}  // namespace

hipError_t launch_gmc_blob_scan(const GmcBlobLaunch &L) {
  if (L.n_frames == 0) return hipSuccess;
  if (L.rec_bytes != 40 && L.rec_bytes != 8) return hipErrorInvalidValue;
  if (!L.flags && !L.centres && !L.blobs && !L.largest && !L.box && !L.info) return hipErrorInvalidValue;
  if (L.pipe) {
    // one plane, no stream table; flags and ONE count (L.centres); a report other than the centres needs the count
    // (L.box: the batch's box array of a pipe with MT_LAYOUT_BOXES, 8-byte aligned — the boxed kernel)
    if (L.stream_off || L.n_streams != 0 || L.blobs || L.largest || ((uintptr_t)L.box & 7u) != 0u || L.info) return hipErrorInvalidValue;
    if (L.report != kGmcBlobReportCentres && L.report != kGmcBlobReportLargest && L.report != kGmcBlobReportVector) return hipErrorInvalidValue;
    if (L.report != kGmcBlobReportCentres && !L.centres) return hipErrorInvalidValue;
  } else {
    if (L.sys_flags != 0 || L.sys_count != 0 || L.report != 0) return hipErrorInvalidValue;
    if (L.keep ? (!L.stream_off || L.n_streams == 0) : (L.stream_off != nullptr || L.n_streams != 0)) return hipErrorInvalidValue;
  }
  if (!check_batch_launch(L)) return hipErrorInvalidValue;
  if (L.k.max_shift < 0 || L.k.max_shift > kGmcMaxShift || L.k.min_share_q8 > 256u) return hipErrorInvalidValue;
  // The kernel indexes the staged keep rows and the planes by these fields: they must be the grid's.
  if (!check_rows(L.k, L.lds_bytes, L.lds_max, gmc_blobs_lds_bytes(L.k.gw, L.k.R)) || L.k.y_lo < 0 || L.k.y_hi > L.k.gh ||
      (size_t)L.k.tile_words != blob_tile_words(L.k.gw, L.k.R) || L.k.W != (L.k.gw + 63) / 64)
    return hipErrorInvalidValue;
  // pipe form: the boxed kernel where the batch has a box array
  return plan_and_launch(
      L, L.pipe, L.flags, L.sys_flags, L.centres, L.sys_count,
      [&](unsigned int grid) {
        hipLaunchKernelGGL(gmc_blobs_clear_kernel, dim3(grid), dim3(256), 0, L.stream, L.flags, L.centres, L.blobs, L.largest, L.box,
                           L.info, L.n_frames);
      },
      [&](auto rec, auto pipe) {
        if constexpr (pipe()) {
          if (L.box) return launch_frames<rec() | kRecBoxed, true>(L);
        }
        return launch_frames<rec(), pipe()>(L);
      });
}

}  // namespace mtgpu
