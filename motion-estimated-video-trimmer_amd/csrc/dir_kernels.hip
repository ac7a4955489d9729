// dir_kernels.hip — the direction filter: the centre scan of src/motion_scanner.cpp:242-292 (without the early return) in
// which a record votes only if the sector of its displacement dst - src is allowed, and the per-frame rose: the counting
// records of each of the eight sectors, whatever is allowed (include/mtgpu_dir.h).
//
//   dir_clear_kernel     zero-fills the non-null outputs ahead of the scan kernel: a frame without side data, and a frame
//                        behind the last stream, reads 0 everywhere.
//   dir_frames_kernel    one workgroup per entry of the scan's work list (plan_frames: the frames with side data, in
//                        stream order).  Surplus workgroups find kNoFrame and leave.
//     stream      with per-stream allow bytes: s = the number of streams that end at or before frame f, a binary search
//                 on workgroup-uniform values; the stream's byte is one scalar load.  Without: the launch's byte.
//     votes       zero the tile; stream the records as the zones kernel does (head peel to a 128-byte line, non-temporal
//                 loads, kDirUnroll in flight per lane).  Per COUNTING record, behind the branch on the threshold and the
//                 bounds that the vote needs anyway: two 24-bit multiplies and compares for the two axis tests, the
//                 sector from the two predicates and the two sign bits, one shift of the allow byte — then the
//                 fire-and-forget `ds_add_u32` of an allowed record.  A record that does not count costs what it costs
//                 in the zones kernel.
//     rose        NOT an LDS atomic per record.  A lane counts its records in eight 8-bit fields of one 64-bit register:
//                 one shifted add per record.  The workgroup streams the frame in pieces of kDirChunk records — a
//                 uniform loop; a frame of up to 131 072 records is one piece — and after each piece the lanes' fields
//                 are summed across the wave (spread to 16-bit fields, DPP inside a row of 16 lanes, four lane reads
//                 across the rows) and lane 0 of each wave adds the non-zero sums to eight LDS words.  A lane sees at
//                 most 130 records of a piece, so no field wraps; the LDS words are 32 bits wide, as the output is.
//     masks       the 64-bit masks of the active cells of every tracked row.
//     centres     the shifted-mask neighbour test with carries across word boundaries.
//   Every output element has one writer after the clear: lane 0 of the frame's workgroup, plain vector stores, no global
//   atomics.
//
// The pipe form (PIPE, include/mtgpu_pipe_dir.h): no clear kernel — the planner answers the frames without side data —
// no stream search, no rose array: every listed frame's workgroup stores the flag and ONE count (the centre count or the
// sector word) on the kernel's one exit, through store_flag / store_centres at the outputs' scope.  With a keep plane
// the rose counts a record only where the keep bit of its destination cell is set, and the active plane is the masked
// one of the zones kernel; the keep words wait in the amask rows they are ANDed into, so the LDS does not grow.
//
// The record loads, the streamers, the row masks, the centre test of a word are those of record_stream.h, instantiated
// here with this kernel's functor; the launch helpers are those of scan_kernels.h.
#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "dir_kernels.hip is written for gfx950 only (wave64, 160 KB LDS)"
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "dir_kernels.h"
#include "record_stream.h"

namespace mtgpu {

namespace {

// ---- the centres: record_stream.h's count_centres, kept as this file's own text.  Called with W and gw as scalars the
// 40-byte pipe form takes 77 SGPRs instead of 76 and the four forms come out in another register order
// (docs/rounds/r24_kernel_fold.md): no fold without identical resource figures.
template <int BLOCK>
__device__ __forceinline__ void count_centres(const unsigned long long *amask, unsigned int *total, const DirK &k, int crows) {
  const int W = k.W;
  const int ntask = crows * W;
  for (int tk = threadIdx.x; tk < ntask; tk += BLOCK) {
    const int r = tk / W, w = tk - r * W;
    const unsigned long long *mr = amask + (size_t)(r + 1) * W;
    if (mr[w] == 0ull) continue;                               // no popcount, no add: most words of most frames
    const unsigned int c = (unsigned int)__popcll(centre_word(mr, w, W, k.gw));
    if (c) atomicAdd(total, c);
  }
}

// ---- one record (src/motion_scanner.cpp:246-268 and the direction test of include/mtgpu_dir.h): threshold, cell,
// bounds as record_stream.h's vote(); then the sector of (dx, dy); a counting record with a sector goes into the lane's
// packed rose; a counting record without a sector, or with an allowed one, votes.
//   axis tests   e: 12 |dy| <= 5 |dx| (E / W), s: 12 |dx| <= 5 |dy| (S / N); |d| <= 65535, so both products fit 24-bit
//                multiplies.  Both hold only for dx == dy == 0.
//   sector       e: 4 sx; s: 2 + 4 sy; neither: 1 + 4 sy + 2 (sx ^ sy)  (sx, sy: the sign bits: 1, 3, 5, 7 clockwise)
// KEEP (the pipe form under a keep plane): `kl` = the staged keep words of the analysed rows (keep row r at kl + r * W).
// The keep bit of the destination cell is read behind the same branch: a record that does not count reads nothing.  A
// record of a keep-0 cell is in no sector of the rose and does not vote (its cell is inactive whatever its votes).
template <bool KEEP = false>
__device__ __forceinline__ void dir_vote(const MvFields m, const DirK &k, int t0, unsigned int *tile, unsigned int allow,
                                         unsigned long long &acc, const unsigned long long *kl = nullptr) {
  const int sdx = m.dst_x - m.src_x, sdy = m.dst_y - m.src_y;  // |.| <= 65535
  const unsigned int dx = (unsigned int)sdx, dy = (unsigned int)sdy;
  // dx*dx < 2^32 exactly; the sum needs 34 bits
  const unsigned long long mag = (unsigned long long)(dx * dx) + (unsigned long long)(dy * dy);
  const int gx = m.dst_x >> k.shift, gy = m.dst_y >> k.shift;
  // 0 <= gx < gw and y_lo <= gy < y_hi (:262) as two unsigned compares (y_hi >= y_lo by construction)
  const bool in = ((unsigned int)gx < (unsigned int)k.gw) & ((unsigned int)(gy - k.y_lo) < (unsigned int)(k.y_hi - k.y_lo));
  // The sector is worked out behind the branch the vote needs anyway: most records of most footage count nothing
  // (they are still, or too slow), and a wave without a counting record skips all of it.  Behind the branch every value
  // is computed for every lane and chosen with selects.
  if (in & (mag >= k.thr)) {
    const unsigned int ax = (unsigned int)(sdx < 0 ? -sdx : sdx), ay = (unsigned int)(sdy < 0 ? -sdy : sdy);
    const bool e = __umul24(12u, ay) <= __umul24(5u, ax), s = __umul24(12u, ax) <= __umul24(5u, ay);
    const unsigned int sx = dx >> 31, sy = dy >> 31;
    const unsigned int diag = 1u | ((sx ^ sy) << 1);
    const unsigned int mid = s ? 2u : diag;
    const unsigned int south = mid | (sy << 2), west = sx << 2;
    const unsigned int sec = e ? west : south;
    const bool none = (dx | dy) == 0u;
    const unsigned int eff = none ? 0xffu : allow;             // no direction to object to
    if constexpr (KEEP) {
      const bool kept = ((kl[(gy - k.y_lo) * k.W + (gx >> 6)] >> (gx & 63)) & 1ull) != 0ull;
      acc += (unsigned long long)((none | !kept) ? 0u : 1u) << (8u * sec);
      if (kept & (((eff >> sec) & 1u) != 0u)) atomicAdd(&tile[(unsigned int)((gy - t0) * k.gw + gx)], 1u);
    } else {
      acc += (unsigned long long)(none ? 0u : 1u) << (8u * sec);
      if (((eff >> sec) & 1u) != 0u) atomicAdd(&tile[(unsigned int)((gy - t0) * k.gw + gx)], 1u);
    }
  }
}

// ---- sums over a wave, every lane active.  Inside a row of 16 lanes with DPP (quad_perm [1,0,3,2], quad_perm
// [2,3,0,1], row_half_mirror, row_mirror: every lane of the row then holds the row's sum), across the four rows with
// four lane reads: a scalar result.
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

// The lanes' packed counters (eight 8-bit fields, each at most 130) -> the eight LDS words, once per wave.  The even
// and the odd fields are spread to four 16-bit fields each: a wave's sum is at most 64 x 130 and stays inside its field.
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

}  // namespace

__global__ __launch_bounds__(256) void dir_clear_kernel(unsigned char *__restrict__ flags, unsigned int *__restrict__ centres,
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

// Waves per SIMD: as zones_frames_kernel — a workgroup is 16 waves, four per SIMD; a 1080p workgroup takes about 31 KB
// of LDS, so the lane limit decides: two workgroups per CU, eight waves per SIMD and so at most 64 VGPRs.
// allows == nullptr: stream_off / n_streams are not read and `allow` serves every frame.
// PIPE: the form for a pipe's staging batch (include/mtgpu_pipe_dir.h) — no stream search: stream_off / n_streams /
// allows are not read and `allow` serves every frame; `rose` is not read (null); `keep` is ONE plane (gh x W words) or
// null; the flag and the ONE count leave through store_flag / store_centres with sys_flags / sys_centres on the kernel's
// one exit, and with report_sectors the count is the sector word lane 0 builds from the eight LDS rose words.  The keep
// words of the analysed rows take no LDS of their own: they are staged into the amask rows they will be ANDed into (keep
// row r <-> mask row r + 1), which are dead until row_masks writes them; the lane that stores a word is the one that
// reads the keep word under it.  keep == nullptr is a workgroup-uniform branch around the staging and around the
// per-record lookup.  !PIPE: keep / sys_* / report_sectors are not read (null / 0).
template <int BLOCK, int UNROLL, int REC, bool PIPE>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void dir_frames_kernel(
    const unsigned char *__restrict__ mv, const WorkItem *__restrict__ work, unsigned int item0, unsigned int n_items, DirK k,
    const unsigned long long *__restrict__ stream_off, unsigned int n_streams, const unsigned char *__restrict__ allows,
    unsigned int allow, unsigned char *__restrict__ flags, unsigned int *__restrict__ centres, unsigned int *__restrict__ rose,
    const unsigned long long *__restrict__ keep, int sys_flags, int sys_centres, int report_sectors) {
  extern __shared__ __attribute__((aligned(16))) unsigned int lds[];
  const unsigned int item = item0 + blockIdx.x;
  if (item >= n_items) return;
  const WorkItem me = load_item(work, item);
  if (me.f == kNoFrame) return;                 // the list has ended (every later entry is past its end too)
  const int tid = threadIdx.x;
  unsigned int *tile = lds;
  unsigned long long *amask = reinterpret_cast<unsigned long long *>(lds + k.tile_words);
  unsigned int *total = reinterpret_cast<unsigned int *>(amask + (size_t)(k.R + 2) * k.W);
  unsigned int *lrose = total + 4;
  const int t0 = max(k.y_lo - 1, 0), t1 = min(k.y_hi + 1, k.gh);
  const int crows = k.y_hi - k.y_lo;

  // The frame's stream: s = the number of streams that end at or before frame f (binary search, workgroup-uniform
  // values: scalar code).  s == n_streams: the frame lies behind the last stream and keeps the zeros of the clear.
  const unsigned int f = __builtin_amdgcn_readfirstlane(me.f);
  [[maybe_unused]] unsigned int tw = (unsigned int)k.tile_words;   // the pipe form only
  if constexpr (!PIPE) {
    if (allows != nullptr) {
      const unsigned int lo = stream_of(stream_off, n_streams, f);
      // in front of the first stream (stream_off[0] > f) the frame belongs to no stream either
      if (lo >= n_streams || stream_off[lo] > (unsigned long long)f) return;
      allow = (unsigned int)allows[lo];
    }
  }
  // ---- zero the tile, the total and the rose
  zero_tile<BLOCK>(tile, k.tile_words);
  if (tid < 12) total[tid] = 0u;                // total[0 .. 3] and the eight rose words behind them
  if constexpr (PIPE) {
    // the keep words of the analysed rows into mask rows 1 .. crows (crows <= R: inside the (R + 2) x W plane); keep row
    // y_lo + r, r < crows, lies inside the gh x W plane
    if (keep != nullptr) {
      const unsigned long long *kp = keep + (size_t)k.y_lo * (size_t)k.W;
      const int nkeep = crows * k.W;
      for (int j = tid; j < nkeep; j += BLOCK) amask[(size_t)k.W + j] = kp[j];
    }
    // The mask plane's offset waits in a VGPR while the records stream (this form takes 52 / 51 VGPRs, 12 to spare under
    // the 64 of eight waves per SIMD): held in an SGPR it is the one value too many there, and the compiler parks it in
    // a VGPR lane itself — an SGPR spill.  Seen with hipcc 7.2.26015 (AMD clang 22.0.0git, roc-7.2.0), where the compact
    // form then reports .sgpr_spill_count 1; the results do not depend on it, only the register use does.  With
    // another compiler read the kernels' resource usage again (docs/rounds/r21_pipe_dir.md has the command line).
    asm volatile("" : "+v"(tw));
  }
  __syncthreads();
  // ---- the votes and the rose (an empty analysed range counts nothing: nothing to read)
  if (crows > 0) {
    for (unsigned long long r = me.r0; r < me.r1; r += kDirChunk) {      // uniform: one piece unless the frame is huge
      const unsigned long long n = (me.r1 - r) < kDirChunk ? (me.r1 - r) : kDirChunk;
      unsigned long long acc = 0ull;
      const auto one = [=, &k, &acc](const MvFields m) { dir_vote(m, k, t0, tile, allow, acc); };
      if constexpr (PIPE) {
        if (keep != nullptr) {
          const unsigned long long *kl = amask + k.W;
          const auto onek = [=, &k, &acc](const MvFields m) { dir_vote<true>(m, k, t0, tile, allow, acc, kl); };
          if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(mv + r * 8ull, n, onek);
          else stream_mv40<BLOCK, UNROLL>(mv + r * 40ull, n, onek);
        } else {
          if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(mv + r * 8ull, n, one);
          else stream_mv40<BLOCK, UNROLL>(mv + r * 40ull, n, one);
        }
      } else {
        if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(mv + r * 8ull, n, one);
        else stream_mv40<BLOCK, UNROLL>(mv + r * 40ull, n, one);
      }
      flush_rose(acc, lrose);
    }
  }
  __syncthreads();
  // ---- the masks, then the centre count
  if constexpr (PIPE) {
    // the plane, the total and the rose are found again from the offset parked in a VGPR above and from
    // R = max(1, crows), which the launch checks
    amask = reinterpret_cast<unsigned long long *>(lds + tw);
    total = reinterpret_cast<unsigned int *>(amask + (size_t)(max(crows, 1) + 2) * k.W);
    lrose = total + 4;
    // an analysed row's word is ANDed with the keep word it overwrites (staged above); halo rows are stored as they come
    const bool masked = keep != nullptr;
    row_masks<BLOCK>(tile, k, t0, t1, k.y_lo - 1, crows + 2, [=, &k](int j, int w, int g, unsigned long long m) {
      unsigned long long *slot = amask + (size_t)j * k.W + w;
      const bool analysed = masked && g >= k.y_lo && g < k.y_hi;
      *slot = analysed ? (m & *slot) : m;
    });
  } else {
    row_masks<BLOCK>(tile, k, t0, t1, k.y_lo - 1, crows + 2, [=, &k](int j, int w, int g, unsigned long long m) {
      amask[(size_t)j * k.W + w] = m;
    });
  }
  __syncthreads();
  count_centres<BLOCK>(amask, &total[0], k, crows);
  __syncthreads();
  if (tid == 0) {
    const unsigned int c = total[0];
    if constexpr (PIPE) {                       // the one exit: a reused pinned block holds the previous batch's values
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
        store_centres(centres, f, word, sys_centres);
      }
      if (flags) store_flag(flags, f, (unsigned char)(c >= k.clust_need ? 1 : 0), sys_flags);
      return;
    }
    if (centres) centres[f] = c;
    if (flags) flags[f] = (unsigned char)(c >= k.clust_need ? 1 : 0);
    if (rose) {
      unsigned int *out = rose + (size_t)f * 8u;
#pragma unroll
      for (int j = 0; j < 8; ++j) out[j] = lrose[j];
    }
  }
}

namespace {

template <int REC, bool PIPE>
hipError_t launch_frames(const DirLaunch &L) {
  auto kern = dir_frames_kernel<kDirBlock, kDirUnroll, REC, PIPE>;
  static std::atomic<unsigned long long> ready{0ull};
  const WorkItem *work = static_cast<const WorkItem *>(L.plan_ws);
  return launch_over_list(kern, ready, L, L.n_frames, [&](unsigned long long i0, unsigned int n) {
    hipLaunchKernelGGL(kern, dim3(n), dim3(kDirBlock), L.lds_bytes, L.stream, L.mv, work, (unsigned int)i0, L.n_frames, L.k,
                       L.stream_off, L.n_streams, L.allows, L.allow, L.flags, L.centres, L.rose, L.keep, L.sys_flags,
                       L.sys_centres, L.report_sectors);
  });
}

}  // namespace

hipError_t launch_dir_scan(const DirLaunch &L) {
  if (L.n_frames == 0) return hipSuccess;
  if (L.rec_bytes != 40 && L.rec_bytes != 8) return hipErrorInvalidValue;
  if (!L.flags && !L.centres && !L.rose) return hipErrorInvalidValue;
  if (L.pipe) {
    if (L.rose || L.allows || (L.report_sectors && !L.centres)) return hipErrorInvalidValue;
  } else {
    if (L.keep || L.sys_flags != 0 || L.sys_centres != 0 || L.report_sectors != 0) return hipErrorInvalidValue;
  }
  if (L.allows ? (!L.stream_off || L.n_streams == 0) : (L.stream_off != nullptr || L.n_streams != 0 || L.allow > 255u))
    return hipErrorInvalidValue;
  if (!check_batch_launch(L) || !check_rows(L.k, L.lds_bytes, L.lds_max, dir_lds_bytes(L.k.gw, L.k.R))) return hipErrorInvalidValue;
  // The pipe form stages the keep rows into the mask plane and indexes them: the block's layout fields must be the grid's.
  // The kernel finds the plane again from R = max(1, y_hi - y_lo).
  if (L.pipe && ((size_t)L.k.tile_words != dir_tile_words(L.k.gw, L.k.R) || L.k.W != (L.k.gw + 63) / 64 || L.k.y_lo < 0 ||
                 L.k.y_hi > L.k.gh || L.k.R != (L.k.y_hi - L.k.y_lo < 1 ? 1 : L.k.y_hi - L.k.y_lo)))
    return hipErrorInvalidValue;
  return plan_and_launch(
      L, L.pipe, L.flags, L.sys_flags, L.centres, L.sys_centres,
      [&](unsigned int grid) {
        hipLaunchKernelGGL(dir_clear_kernel, dim3(grid), dim3(256), 0, L.stream, L.flags, L.centres, L.rose, L.n_frames);
      },
      [&](auto rec, auto pipe) { return launch_frames<rec(), pipe()>(L); });
}

}  // namespace mtgpu
