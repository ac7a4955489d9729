// gmc_kernels.hip — global-motion compensation: the centre scan of src/motion_scanner.cpp:242-292 (without the early
// return) on the residuals of every frame's dominant vector.  check_frame thresholds each vector's own magnitude
// (:246-251), so a moving camera makes every record pass; here the per-axis mode of the frame's displacements is taken
// first and subtracted (include/mtgpu_gmc.h: the semantics, all integer and exact).
//
//   gmc_clear_kernel    zero-fills the non-null outputs ahead of the scan kernel: a frame without side data reads 0
//                       everywhere, all fields of its info included.
//   gmc_frames_kernel   one workgroup per entry of the scan's work list (plan_frames: the frames with side data).
//                       Surplus workgroups find kNoFrame and leave.
//     estimate    zero the tile and the histograms; stream the records (record_stream.h's streamers, as the siblings do)
//                 with a functor that does the bounds test of :262 and, for a record inside, one add per axis into
//                 hist[d + max_shift] where |d| <= max_shift.  n_in is counted in a register per lane and summed once.
//                 The adds of a wave are aggregated: on the frames this kernel is for (a pan) every record of a wave
//                 hits ONE bin per axis, 64 same-address LDS atomics per instruction.  Each lane compares its bin with
//                 the first active lane's; the leader adds the popcount of the agreeing lanes once, a lane that
//                 disagrees adds for itself.  -DMTGPU_GMC_NAIVE_HIST: one add per lane (the A/B of docs/rounds/r10_gmc.md).
//     pick        wave 0: lane l takes the candidates l, l + 64, ... of the walk 0, -1, +1, -2, +2, ... (at most 255 per
//                 axis), key = count << 8 | (255 - walk index), a max-reduction across the wave: the largest count wins,
//                 among equal counts the earliest of the walk.  Lane 0 applies the support test and leaves gx, gy, the
//                 modes and their counts in LDS.
//     vote        stream the same records a second time: residual = displacement - (gx, gy), squares in 64 bits (|r| can
//                 reach 65 662), threshold, destination cell, one `ds_add_u32` per kept record.
//     masks, centres   row_masks and centre_word of record_stream.h on one plane, as the zones kernel does.
//   Every output element has one writer after the clear: lane 0 of the frame's workgroup, plain vector stores, no global
//   atomics.
//
// The pipe form (PIPE, include/mtgpu_pipe_gmc.h): no clear kernel — the planner answers the frames without side data and
// every listed frame's workgroup stores the flag and ONE count on the kernel's one exit, through store_flag /
// store_centres at the outputs' scope; no info.  With a keep plane the estimate counts a record only where the keep bit
// of its destination cell is set, and the active plane is the masked one of the zones kernel.  The keep words of the
// analysed rows take no LDS of their own: they are staged into the amask rows they will be ANDed into (keep row r <->
// mask row r + 1), which are dead until row_masks writes them; row_masks visits every (row, word) once, and the lane that
// stores a word is the one that reads the keep word under it.  keep == nullptr is a workgroup-uniform branch around the
// staging and around the per-record lookup.
//
// record_stream.h is used as it is; nothing here changes the siblings' device code.  Both passes read with the
// streaming hint: with or without it the second pass comes from HBM (docs/rounds/r10_gmc.md).
#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "gmc_kernels.hip is written for gfx950 only (wave64, 160 KB LDS)"
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "gmc_kernels.h"
#include "record_stream.h"

namespace mtgpu {

namespace {

#ifdef MTGPU_GMC_NAIVE_HIST
constexpr bool kGmcAggregate = false;
#else
constexpr bool kGmcAggregate = true;
#endif

// One add into bin `bin` of `h` for every lane with `on`.  Aggregated: the lanes whose bin equals the first active
// lane's are added by that lane in one atomic; the others add for themselves.
__device__ __forceinline__ void hist_add(unsigned int *h, int bin, bool on) {
  if (!on) return;
  if constexpr (kGmcAggregate) {
    const int lead = __builtin_amdgcn_readfirstlane(bin);     // the first active lane's bin
    const bool same = bin == lead;
    const unsigned long long grp = __ballot(same);            // among the active lanes; the first one is in it
    if (same) {
      if ((int)__lane_id() == __ffsll((long long)grp) - 1) atomicAdd(&h[lead], (unsigned int)__popcll(grp));
    } else {
      atomicAdd(&h[bin], 1u);
    }
  } else {
    atomicAdd(&h[bin], 1u);
  }
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

}  // namespace

__global__ __launch_bounds__(256) void gmc_clear_kernel(unsigned char *__restrict__ flags, unsigned int *__restrict__ centres,
                                                        unsigned int *__restrict__ info, unsigned int n) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull) {
    if (flags) flags[i] = (unsigned char)0;
    if (centres) centres[i] = 0u;
    if (info) {
#pragma unroll
      for (int j = 0; j < kGmcInfoWords; ++j) info[i * (unsigned long long)kGmcInfoWords + j] = 0u;
    }
  }
}

// Waves per SIMD as for the zones kernel: 1080p takes about 35 KB of LDS, the lane limit decides (two workgroups per CU,
// eight waves per SIMD, at most 64 VGPRs); the 4K workgroup sits alone on its CU.
// PIPE: the form for a pipe's staging batch — `info` is not read (null), `keep` is ONE plane (gh x W words) or null, the
// results leave through store_flag / store_centres with sys_flags / sys_centres, and with report_vector the count is the
// applied vector, (uint16)gx | (uint16)gy << 16.  !PIPE: keep / sys_* / report_vector are not read (null / 0).
template <int BLOCK, int UNROLL, int REC, bool PIPE>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void gmc_frames_kernel(
    const unsigned char *__restrict__ mv, const WorkItem *__restrict__ work, unsigned int item0, unsigned int n_items, GmcK k,
    unsigned char *__restrict__ flags, unsigned int *__restrict__ centres, unsigned int *__restrict__ info,
    const unsigned long long *__restrict__ keep, int sys_flags, int sys_centres, int report_vector) {
  extern __shared__ __attribute__((aligned(16))) unsigned int lds[];
  const unsigned int item = item0 + blockIdx.x;
  if (item >= n_items) return;
  const WorkItem me = load_item(work, item);
  if (me.f == kNoFrame) return;                 // the list has ended (every later entry is past its end too)
  const int tid = threadIdx.x;
  unsigned int *tile = lds;
  unsigned long long *amask = reinterpret_cast<unsigned long long *>(lds + k.tile_words);
  unsigned int *hx = reinterpret_cast<unsigned int *>(amask + (size_t)(k.R + 2) * k.W);
  unsigned int *hy = hx + kGmcHistBins;
  unsigned int *res = hy + kGmcHistBins;
  const int t0 = max(k.y_lo - 1, 0), t1 = min(k.y_hi + 1, k.gh);
  const int crows = k.y_hi - k.y_lo;
  const int ms = k.max_shift;
  const unsigned int f = __builtin_amdgcn_readfirstlane(me.f);
  const unsigned char *recs = mv + me.r0 * (unsigned long long)REC;
  const unsigned long long nrec = me.r1 - me.r0;

  // ---- zero the tile, the histograms and the result words
  zero_tile<BLOCK>(tile, k.tile_words);
  if (tid < 2 * kGmcHistBins + 8) hx[tid] = 0u;                // hx, hy and res are contiguous
  if constexpr (PIPE) {
    // the keep words of the analysed rows into mask rows 1 .. crows (crows <= R: inside the (R + 2) x W plane); keep row
    // y_lo + r, r < crows, lies inside the gh x W plane
    if (keep != nullptr) {
      const unsigned long long *kp = keep + (size_t)k.y_lo * (size_t)k.W;
      const int nkeep = crows * k.W;
      for (int j = tid; j < nkeep; j += BLOCK) amask[(size_t)k.W + j] = kp[j];
    }
  }
  __syncthreads();
  // ---- the estimate (an empty analysed range counts nothing: nothing to read)
  if (crows > 0) {
    unsigned int mine = 0u;
    const auto one = [=, &k, &mine](const MvFields m) {
      const int gx = m.dst_x >> k.shift, gy = m.dst_y >> k.shift;
      const bool in = ((unsigned int)gx < (unsigned int)k.gw) & ((unsigned int)(gy - k.y_lo) < (unsigned int)(k.y_hi - k.y_lo));
      const int dx = m.dst_x - m.src_x, dy = m.dst_y - m.src_y;
      mine += in ? 1u : 0u;
      // |d| <= max_shift as one unsigned compare
      hist_add(hx, dx + ms, in && (unsigned int)(dx + ms) <= (unsigned int)(2 * ms));
      hist_add(hy, dy + ms, in && (unsigned int)(dy + ms) <= (unsigned int)(2 * ms));
    };
    if constexpr (PIPE) {
      if (keep != nullptr) {
        // counted: inside the bounds AND the keep bit of the destination cell (one LDS read per counted record; a record
        // outside the bounds reads nothing)
        const unsigned long long *kl = amask + k.W;
        const auto onek = [=, &k, &mine](const MvFields m) {
          const int gx = m.dst_x >> k.shift, gy = m.dst_y >> k.shift;
          bool in = ((unsigned int)gx < (unsigned int)k.gw) & ((unsigned int)(gy - k.y_lo) < (unsigned int)(k.y_hi - k.y_lo));
          if (in) in = ((kl[(gy - k.y_lo) * k.W + (gx >> 6)] >> (gx & 63)) & 1ull) != 0ull;
          const int dx = m.dst_x - m.src_x, dy = m.dst_y - m.src_y;
          mine += in ? 1u : 0u;
          hist_add(hx, dx + ms, in && (unsigned int)(dx + ms) <= (unsigned int)(2 * ms));
          hist_add(hy, dy + ms, in && (unsigned int)(dy + ms) <= (unsigned int)(2 * ms));
        };
        if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(recs, nrec, onek);
        else stream_mv40<BLOCK, UNROLL>(recs, nrec, onek);
      } else {
        if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(recs, nrec, one);
        else stream_mv40<BLOCK, UNROLL>(recs, nrec, one);
      }
    } else {
      if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(recs, nrec, one);
      else stream_mv40<BLOCK, UNROLL>(recs, nrec, one);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
    if ((tid & 63) == 0 && mine) atomicAdd(&res[1], mine);
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
  // ---- the votes on the residuals
  int vrows = crows;
  // pipe form: the test is taken anew (else its 64-bit result is held across the estimate, in VGPR lanes: an SGPR spill)
  if constexpr (PIPE) vrows = __builtin_amdgcn_readfirstlane(crows);
  if (vrows > 0) {
    const auto one = [=, &k](const MvFields m) {
      const int rx = (m.dst_x - m.src_x) - cgx, ry = (m.dst_y - m.src_y) - cgy;   // |r| <= 65535 + 127
      const unsigned int ax = (unsigned int)(rx < 0 ? -rx : rx), ay = (unsigned int)(ry < 0 ? -ry : ry);
      // a square can exceed 2^32: 64-bit products
      const unsigned long long mag = (unsigned long long)ax * ax + (unsigned long long)ay * ay;
      const int gx = m.dst_x >> k.shift, gy = m.dst_y >> k.shift;
      const bool in = ((unsigned int)gx < (unsigned int)k.gw) & ((unsigned int)(gy - k.y_lo) < (unsigned int)(k.y_hi - k.y_lo));
      if (in && mag >= k.thr) atomicAdd(&tile[(unsigned int)((gy - t0) * k.gw + gx)], 1u);
    };
    if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(recs, nrec, one);
    else stream_mv40<BLOCK, UNROLL>(recs, nrec, one);
  }
  __syncthreads();
  // ---- the masks, then the centre count (the zones kernel's, one plane)
  if constexpr (PIPE) {
    // an analysed row's word is ANDed with the keep word it overwrites (staged above); halo rows are stored as they come
    const bool masked = keep != nullptr;
    row_masks<BLOCK>(tile, k, t0, t1, k.y_lo - 1, crows + 2, [=, &k](int j, int w, int g, unsigned long long m) {
      unsigned long long *slot = amask + (size_t)j * k.W + w;
      const bool analysed = masked && g >= k.y_lo && g < k.y_hi;
      *slot = analysed ? (m & *slot) : m;
    });
  } else {
    row_masks<BLOCK>(tile, k, t0, t1, k.y_lo - 1, crows + 2,
                     [=, &k](int j, int w, int g, unsigned long long m) { amask[(size_t)j * k.W + w] = m; });
  }
  __syncthreads();
  count_centres<BLOCK>(amask, &res[0], k.W, k.gw, crows);
  __syncthreads();
  if (tid == 0) {
    const unsigned int c = res[0];
    if constexpr (PIPE) {                                       // the one exit: a reused pinned block holds the previous batch's values
      if (centres) store_centres(centres, f, report_vector ? ((res[2] & 0xffffu) | (res[3] << 16)) : c, sys_centres);
      if (flags) store_flag(flags, f, (unsigned char)(c >= k.clust_need ? 1 : 0), sys_flags);
      return;
    }
    if (centres) centres[f] = c;
    if (flags) flags[f] = (unsigned char)(c >= k.clust_need ? 1 : 0);
    if (info) {
      unsigned int *o = info + (unsigned long long)f * kGmcInfoWords;   // mt_gmc_info: int16 gx, gy, mode_x, mode_y; u32 n_in, n_x, n_y
      o[0] = (res[2] & 0xffffu) | (res[3] << 16);
      o[1] = (res[4] & 0xffffu) | (res[5] << 16);
      o[2] = res[1];
      o[3] = res[6];
      o[4] = res[7];
    }
  }
}

namespace {

template <int REC, bool PIPE>
hipError_t launch_frames(const GmcLaunch &L) {
  auto kern = gmc_frames_kernel<kGmcBlock, kGmcUnroll, REC, PIPE>;
  static std::atomic<unsigned long long> ready{0ull};
  const WorkItem *work = static_cast<const WorkItem *>(L.plan_ws);
  return launch_over_list(kern, ready, L, L.n_frames, [&](unsigned long long i0, unsigned int n) {
    hipLaunchKernelGGL(kern, dim3(n), dim3(kGmcBlock), L.lds_bytes, L.stream, L.mv, work, (unsigned int)i0, L.n_frames, L.k,
                       L.flags, L.centres, L.info, L.keep, L.sys_flags, L.sys_centres, L.report_vector);
  });
}

}  // namespace

hipError_t launch_gmc_scan(const GmcLaunch &L) {
  if (L.n_frames == 0) return hipSuccess;
  if (L.rec_bytes != 40 && L.rec_bytes != 8) return hipErrorInvalidValue;
  if (!L.flags && !L.centres && !L.info) return hipErrorInvalidValue;
  if (L.pipe) {
    if (L.info || (L.report_vector && !L.centres)) return hipErrorInvalidValue;
  } else {
    if (L.keep || L.sys_flags != 0 || L.sys_centres != 0 || L.report_vector != 0) return hipErrorInvalidValue;
  }
  if (!check_batch_launch(L) || !check_rows(L.k, L.lds_bytes, L.lds_max, gmc_lds_bytes(L.k.gw, L.k.R))) return hipErrorInvalidValue;
  if (L.k.max_shift < 0 || L.k.max_shift > kGmcMaxShift || L.k.min_share_q8 > 256u) return hipErrorInvalidValue;
  // The pipe form stages the keep rows into the mask plane and indexes them: the block's layout fields must be the grid's.
  if (L.pipe && ((size_t)L.k.tile_words != gmc_tile_words(L.k.gw, L.k.R) || L.k.W != (L.k.gw + 63) / 64 || L.k.y_lo < 0 || L.k.y_hi > L.k.gh))
    return hipErrorInvalidValue;
  return plan_and_launch(
      L, L.pipe, L.flags, L.sys_flags, L.centres, L.sys_centres,
      [&](unsigned int grid) {
        hipLaunchKernelGGL(gmc_clear_kernel, dim3(grid), dim3(256), 0, L.stream, L.flags, L.centres, L.info, L.n_frames);
      },
      [&](auto rec, auto pipe) { return launch_frames<rec(), pipe()>(L); });
}

}  // namespace mtgpu
