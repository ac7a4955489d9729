// sweep_kernels.hip — the centre counts of MotionScanner::check_frame (src/motion_scanner.cpp:217-295, the `clusters`
// counter of :272-294 without its early return) for EVERY pair (MV_THRESHOLD_SQ, VECTORS_NEEDED) of a sensitivity
// study, from one read of a frame's records.  The thresholds are nested (a record that passes ceil(T) passes every
// smaller one, :251) and a cell's vote count answers every VECTORS_NEEDED at once (:282), so only the cluster test is
// per-setting work, and it runs over LDS.
//
//   sweep_clear_kernel    zero-fills the whole output block ahead of the scan: frames without side data (:219-221)
//                         and frames the work list leaves out keep that 0 in every setting.
//   sweep_frames_kernel   one workgroup per entry of the scan's work list (plan_frames: the frames with side data, in
//                         stream order).  No slicing of large frames and no grouping of small ones: a launch of a few
//                         frames, or of very small frames, does not fill the chip.
//     phase 0  zero the tiles and the totals
//     phase 1  stream the records as the scan does (REC 40: bytes 4..15 of each AVMotionVector, REC 8: compact
//              records in 16-byte pairs).  A record that votes (:246-262, the cell and bounds test of the scan's
//              keep_and_cell) makes ONE fire-and-forget `ds_add_u32`, whatever the number of thresholds: into the
//              tile of the HIGHEST threshold it passes.  32-bit counters: exact for any frame below 2^32 records
//              (the reference's u8 saturation at 255, :265-266, is unobservable: only `>= vectors_needed` with
//              vectors_needed <= 255 is ever tested).
//     fold     votes of threshold i = tiles i .. T-1 added up, in place: one pass over the cells, lane-private
//     phase 2  per threshold, per chunk of rows: the activity masks of ALL vector levels from one read of the
//              counters (four lanes per 64-cell word, the cells held in registers across the levels), then the
//              shifted-mask 4-neighbour test of the scan's count_centres over every (level, row, word)
//   thread i * n_vec + v stores setting (threshold i, level v): d_centres[(t * n_vec + v) * n_frames + f], t the
//   caller's index of the pass's threshold i.  Plain vector stores; system-scope when the block is not device memory.
//
// A grid whose thresholds do not fit LDS together is swept in several launches, each over a contiguous run of the
// sorted thresholds (mtgpu_api.hip, sweep_plan): every launch reads the records again.
//
// The record loads, the streamers (with vote<NT> as their functor), the centre test of a word and the result store are
// those of record_stream.h, shared with activity_kernels.hip and zones_kernels.hip; the launch helpers are those of
// scan_kernels.h.  vote<NT> and the multi-level row_masks are this file's own.  A change to the shared header must leave
// this file's device assembly as it was, or be timed against the build before it.
#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "sweep_kernels.hip is written for gfx950 only (wave64, 160 KB LDS, sc1 write-through stores)"
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "sweep_kernels.h"
#include "record_stream.h"

namespace mtgpu {

namespace {

// The workgroup's view of its frame's grid: tracked rows [t0, t1) = the analysed rows [y_lo, y_hi) and one halo row
// each side (inside the grid), centres [y_lo, y_hi).
struct Rows { int t0, t1; };

// One record (src/motion_scanner.cpp:246-268): threshold, cell, bounds — exactly the scan's keep_and_cell — then one
// vote into the tile of the highest threshold of the pass the record passes.  NT: thresholds the kernel compares
// against (k.thr is padded with ~0, which no |d|^2 reaches).
template <int NT>
__device__ __forceinline__ void vote(const MvFields m, const SweepK &k, const Rows &b, unsigned int *tiles) {
  const unsigned int dx = (unsigned int)(m.dst_x - m.src_x);   // |dx| <= 65535
  const unsigned int dy = (unsigned int)(m.dst_y - m.src_y);
  // dx*dx < 2^32 exactly; the sum needs 34 bits
  const unsigned long long mag = (unsigned long long)(dx * dx) + (unsigned long long)(dy * dy);
  const int gx = m.dst_x >> k.shift, gy = m.dst_y >> k.shift;
  // 0 <= gx < gw and y_lo <= gy < y_hi (:262) as two unsigned compares (y_hi >= y_lo by construction)
  const bool in = ((unsigned int)gx < (unsigned int)k.gw) & ((unsigned int)(gy - k.y_lo) < (unsigned int)(k.y_hi - k.y_lo));
  unsigned int passed = 0u;                                    // thresholds are ascending: the first `passed` of them
#pragma unroll
  for (int i = 0; i < NT; ++i) passed += (mag >= k.thr[i]) ? 1u : 0u;
  if (in && passed != 0u)
    atomicAdd(&tiles[(size_t)(passed - 1u) * (unsigned int)k.tile_words + (unsigned int)((gy - b.t0) * k.gw + gx)], 1u);
}

// ---- fold: tile i becomes the votes of threshold i = the sum of tiles i .. n_thr-1.  Every lane owns its 16-byte
// columns through all tiles: no barrier between the tiles.
template <int BLOCK>
__device__ __forceinline__ void fold_tiles(unsigned int *tiles, const SweepK &k) {
  const int n4 = k.tile_words >> 2;
  u32x4 *t4 = reinterpret_cast<u32x4 *>(tiles);
  for (int c = threadIdx.x; c < n4; c += BLOCK) {
    u32x4 acc = t4[(size_t)(k.n_thr - 1) * n4 + c];
    for (int i = k.n_thr - 2; i >= 0; --i) {
      acc += t4[(size_t)i * n4 + c];
      t4[(size_t)i * n4 + c] = acc;
    }
  }
}

// ---- phase 2a: the 64-bit masks of active cells of grid rows [g0, g0 + nrows), one plane per vector level: plane v,
// mask row j <-> grid row g0 + j.  Rows outside the tracked rows and cells outside the grid are inactive at every
// level, level 0 included (:282 with vectors_needed == 0: every cell OF THE GRID is active).
// Four lanes per (mask row, word), 16 cells each, as the scan's row_masks (record_stream.h has the single-level form;
// this one holds the cells in registers across the levels): the cells are read ONCE, in a rotated order
// (the 64 lanes of a wave hit 64 different LDS banks per step), and compared against each level in registers.
template <int BLOCK>
__device__ __forceinline__ void row_masks(const unsigned int *cnt, unsigned long long *mask, const SweepK &k, const Rows &b,
                                          int g0, int nrows) {
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
    const bool live = tk < ntask && g >= b.t0 && g < b.t1 && ncell > 0;
    const int last = min(ncell, 16) - 1;
    unsigned int val[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) val[u] = 0u;
    if (live) {
      const unsigned int *row = cnt + (size_t)(g - b.t0) * k.gw + w * 64 + sub * 16;
#pragma unroll
      for (int u = 0; u < 16; ++u) val[u] = row[min((u + rot) & 15, last)];   // always inside the row
    }
    const unsigned int valid = live ? ((2u << last) - 1u) : 0u;               // bits 0 .. last
    for (int v = 0; v < k.n_vec; ++v) {
      const unsigned int need = k.vec[v];
      unsigned int q = 0u;                                     // bit u: the cell read u-th, i.e. cell (u + rot) & 15
#pragma unroll
      for (int u = 0; u < 16; ++u) q |= (val[u] >= need ? 1u : 0u) << u;
      q = ((q << rot) | (q >> (16 - rot))) & 0xffffu & valid;  // rotate the 16 bits into cell order
      unsigned long long m = (unsigned long long)q << (sub * 16);
      m |= __shfl_xor(m, 1);
      m |= __shfl_xor(m, 2);
      if (tk < ntask && sub == 0) mask[((size_t)v * k.mask_rows + j) * W + w] = m;
    }
  }
}

// ---- phase 2b: centre cells with an active 4-neighbour (:277-293), one task per (level, centre row, word): centre
// row r <-> mask row r + 1 of the level's plane; x in [1, gw-2] (:280); neighbours across word and row boundaries;
// outside the grid: inactive.  The scan's count_centres, with the count added to the setting's total in LDS.
template <int BLOCK>
__device__ __forceinline__ void count_centres(const unsigned long long *mask, unsigned int *totals, const SweepK &k, int nrows) {
  const int W = k.W;
  const int per = nrows * W, ntask = k.n_vec * per;
  for (int tk = threadIdx.x; tk < ntask; tk += BLOCK) {
    const int v = tk / per, rw = tk - v * per;
    const int r = rw / W, w = rw - r * W;
    const unsigned long long *mr = mask + ((size_t)v * k.mask_rows + r + 1) * W;
    if (mr[w] == 0ull) continue;                               // no popcount, no add: most words of most frames
    const unsigned int c = (unsigned int)__popcll(centre_word(mr, w, W, k.gw));
    if (c) atomicAdd(&totals[v], c);
  }
}

}  // namespace

__global__ __launch_bounds__(256) void sweep_clear_kernel(unsigned int *__restrict__ centres, unsigned long long n, int sys) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull)
    store_result(&centres[i], 0u, sys);
}

template <int BLOCK, int UNROLL, int REC, int NT>
__global__ __launch_bounds__(BLOCK) void sweep_frames_kernel(
    const unsigned char *__restrict__ mv, const WorkItem *__restrict__ work, unsigned int item0, unsigned int n_items,
    SweepK k, unsigned int *__restrict__ centres, unsigned int n_frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned int lds[];
  const unsigned int item = item0 + blockIdx.x;
  if (item >= n_items) return;
  const WorkItem me = load_item(work, item);
  if (me.f == kNoFrame) return;                 // the list has ended (every later entry is past its end too)
  const int tid = threadIdx.x;
  unsigned int *tiles = lds;
  unsigned long long *mask = reinterpret_cast<unsigned long long *>(lds + (size_t)k.n_thr * k.tile_words);
  unsigned int *totals = reinterpret_cast<unsigned int *>(mask + (size_t)k.n_vec * k.mask_rows * k.W);
  const Rows b = {max(k.y_lo - 1, 0), min(k.y_hi + 1, k.gh)};

  // ---- phase 0
  zero_tile<BLOCK>(tiles, k.n_thr * k.tile_words);
  if (tid < kSweepMaxThr * kSweepMaxVec) totals[tid] = 0u;
  __syncthreads();

  // ---- phase 1 (an empty analysed range keeps nothing: nothing to read)
  if (k.y_hi > k.y_lo) {
    const auto one = [=, &k](const MvFields m) { vote<NT>(m, k, b, tiles); };
    if constexpr (REC == 8) stream_compact<BLOCK, UNROLL>(mv + me.r0 * 8ull, me.r1 - me.r0, one);
    else stream_mv40<BLOCK, UNROLL>(mv + me.r0 * 40ull, me.r1 - me.r0, one);
  }
  __syncthreads();
  if (k.n_thr > 1) {
    fold_tiles<BLOCK>(tiles, k);
    __syncthreads();
  }

  // ---- phase 2: chunks of centre rows [y_lo + q0, y_lo + q0 + qn); mask row j <-> grid row y_lo + q0 - 1 + j
  const int crows = k.y_hi - k.y_lo;
  for (int i = 0; i < k.n_thr; ++i) {
    const unsigned int *cnt = tiles + (size_t)i * k.tile_words;
    for (int q0 = 0; q0 < crows; q0 += k.chunk_rows) {
      const int qn = min(k.chunk_rows, crows - q0);
      row_masks<BLOCK>(cnt, mask, k, b, k.y_lo + q0 - 1, qn + 2);
      __syncthreads();
      count_centres<BLOCK>(mask, totals + i * kSweepMaxVec, k, qn);
      __syncthreads();                                   // the masks are rewritten next
    }
  }

  if (tid < k.n_thr * k.n_vec) {
    const int i = tid / k.n_vec, v = tid - i * k.n_vec;
    const unsigned long long at = ((unsigned long long)k.out_t[i] * (unsigned int)k.n_vec + (unsigned int)v) * n_frames + me.f;
    store_result(&centres[at], totals[i * kSweepMaxVec + v], k.sys);
  }
}

namespace {

template <int REC, int NT>
hipError_t launch_pass(const SweepLaunch &L, const SweepK &k) {
  auto kern = sweep_frames_kernel<kSweepBlock, kSweepUnroll, REC, NT>;
  static std::atomic<unsigned long long> ready{0ull};
  const WorkItem *work = static_cast<const WorkItem *>(L.plan_ws);
  return launch_over_list(kern, ready, L, L.n_frames, [&](unsigned long long i0, unsigned int n) {
    hipLaunchKernelGGL(kern, dim3(n), dim3(kSweepBlock), L.lds_bytes, L.stream, L.mv, work, (unsigned int)i0, L.n_frames, k,
                       L.centres, L.n_frames);
  });
}

// The instantiations: two record forms x 1, 2, 4 or 8 threshold compares per record.
template <int REC>
hipError_t launch_pass_nt(const SweepLaunch &L, const SweepK &k) {
  if (k.n_thr <= 1) return launch_pass<REC, 1>(L, k);
  if (k.n_thr <= 2) return launch_pass<REC, 2>(L, k);
  if (k.n_thr <= 4) return launch_pass<REC, 4>(L, k);
  return launch_pass<REC, 8>(L, k);
}

}  // namespace

hipError_t launch_sweep_scan(const SweepLaunch &L) {
  if (L.n_frames == 0) return hipSuccess;
  if (L.rec_bytes != 40 && L.rec_bytes != 8) return hipErrorInvalidValue;
  if (!L.centres || !check_batch_launch(L)) return hipErrorInvalidValue;
  if (L.n_thr_all < 1 || L.n_thr_all > kSweepMaxThr || L.k.n_vec < 1 || L.k.n_vec > kSweepMaxVec || L.thr_per_pass < 1 ||
      L.lds_bytes > L.lds_max)
    return hipErrorInvalidValue;
  {
    const unsigned long long n = (unsigned long long)L.n_thr_all * (unsigned long long)L.k.n_vec * L.n_frames;
    hipLaunchKernelGGL(sweep_clear_kernel, dim3(clear_grid(n)), dim3(256), 0, L.stream, L.centres, n, L.k.sys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  // flags / centres null: the planner answers nothing itself (the block is zero already)
  hipError_t e = plan_work_list(L, nullptr, 0, nullptr, 0);
  if (e != hipSuccess) return e;
  for (int t0 = 0; t0 < L.n_thr_all; t0 += L.thr_per_pass) {
    SweepK k = L.k;
    k.n_thr = L.n_thr_all - t0 < L.thr_per_pass ? L.n_thr_all - t0 : L.thr_per_pass;
    for (int i = 0; i < kSweepMaxThr; ++i) {
      k.thr[i] = i < k.n_thr ? L.thr_sorted[t0 + i] : ~0ull;
      k.out_t[i] = i < k.n_thr ? L.thr_index[t0 + i] : 0u;
    }
    e = L.rec_bytes == 8 ? launch_pass_nt<8>(L, k) : launch_pass_nt<40>(L, k);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace mtgpu
