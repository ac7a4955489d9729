// blob_label.h — the labelling of a centre plane in LDS: union-find over a dead vote tile, five passes (init, unite,
// flatten, winner, box) as `__device__ __forceinline__` functions.  The ONE text of them: blobs_frames_kernel
// (blobs_kernels.hip) and gmc_blobs_frames_kernel (gmc_blobs_kernels.hip, on the residual centres) both call it, in
// every form.  find_root and unite have no iteration cap, so an edit here is made once and is then held, for all three
// labelling kernels (resident, pipe, compensated), by tests/test_gpu_blob_planes.py: random connectivity (percolation,
// mazes, combs), every kernel against the model and the kernels against each other, the smallest grid first.
//
//   cpl     crows x W u64   the centre plane: bit x & 63 of word x >> 6 of row r is the centre (x, y_lo + r)
//   L       crows x gw u32  the labels, word r * gw + x.  A root holds kRoot | (cells - 1), every other cell the index
//                           of a cell of its component with a smaller index
//   total   8 u32           [0] centres, [1] blobs, [2..3] the winner's key (u64, 8-byte aligned), [4..7] its box:
//                           min x, min r, max x, max r ([4], [5] start at 0xffffffff, the rest at 0)
// Each pass is followed by a workgroup barrier in the caller.  No pass has a barrier inside; every trip count depends
// on the wave alone.  BLOCK is a multiple of 64: a wave owns one 64-cell word of one row, lane = bit.
// Internal; included after record_stream.h; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mtgpu {
namespace blob_label {

constexpr unsigned int kRoot = 0x80000000u;    // label word of a root: kRoot | (cells of the tree - 1)

// The root of cell x: labels below kRoot are cell indices smaller than the cell that holds them.
__device__ __forceinline__ unsigned int find_root(unsigned int *L, unsigned int x) {
  for (;;) {
    const unsigned int v = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (v & kRoot) return x;
    x = v;
  }
}

// Joins the trees of cells a and b.  Runs concurrently in every lane; only roots are linked, always towards the smaller
// index.  When the atomic finds that `a` has been linked by another lane in the meantime, label[a] is min(old, b) now,
// and old and b are what remains to be joined.
__device__ __forceinline__ void unite(unsigned int *L, unsigned int a, unsigned int b) {
  for (;;) {
    a = find_root(L, a);
    b = find_root(L, b);
    if (a == b) return;
    if (a < b) { const unsigned int t = a; a = b; b = t; }
    const unsigned int old = atomicMin(&L[a], b);
    if (old & kRoot) return;
    a = old;
  }
}

// f(r, w, cw, tw) for every non-empty word cw = cpl[tw] of the centre plane, tw = r * W + w; a wave per word, lane =
// bit.  The trip count depends on the wave alone.
template <int BLOCK, class F>
__device__ __forceinline__ void for_centre_words(const unsigned long long *cpl, int crows, int W, F f) {
  const int nw = crows * W;
  for (int tw = (int)(threadIdx.x >> 6); tw < nw; tw += BLOCK / 64) {
    const unsigned long long cw = cpl[tw];
    if (cw == 0ull) continue;
    const int r = tw / W;
    f(r, tw - r * W, cw, tw);
  }
}

// init: the first cell of a horizontal run is a root, the others point at it.  Column 0 is never a centre, so the scan
// to the left ends at a clear bit; `ww >= 0` bounds it all the same.
template <int BLOCK>
__device__ __forceinline__ void init(const unsigned long long *cpl, int crows, int W, int gw, unsigned int *L, int lane) {
  for_centre_words<BLOCK>(cpl, crows, W, [&](int r, int w, unsigned long long cw, int tw) {
    if (((cw >> lane) & 1ull) == 0ull) return;
    const unsigned long long below = ~cw & ((1ull << lane) - 1ull);        // clear bits to the left of this cell, in its word
    int xs;
    if (below != 0ull) {
      xs = w * 64 + 64 - __clzll((long long)below);
    } else {
      xs = w * 64;
      for (int ww = w - 1; ww >= 0; --ww) {
        const unsigned long long nz = ~cpl[tw - w + ww];
        if (nz != 0ull) { xs = ww * 64 + 64 - __clzll((long long)nz); break; }
        xs = ww * 64;
      }
    }
    const int x = w * 64 + lane;
    L[r * gw + x] = (x == xs) ? kRoot : (unsigned int)(r * gw + xs);
  });
}

// unite: the first cell of every segment in which this row's centres lie under the row above's (per word: a segment
// that crosses a word seam is joined twice)
template <int BLOCK>
__device__ __forceinline__ void unite_rows(const unsigned long long *cpl, int crows, int W, int gw, unsigned int *L, int lane) {
  for_centre_words<BLOCK>(cpl, crows, W, [&](int r, int w, unsigned long long cw, int tw) {
    if (r == 0) return;
    const unsigned long long both = cw & cpl[tw - W];
    const unsigned long long first = both & ~(both << 1);
    if ((first >> lane) & 1ull) {
      const unsigned int i = (unsigned int)(r * gw + w * 64 + lane);
      unite(L, i, i - (unsigned int)gw);
    }
  });
}

// flatten and count: a cell that is no root stores its root and adds 1 to it — one add per (wave, distinct root)
template <int BLOCK>
__device__ __forceinline__ void flatten(const unsigned long long *cpl, int crows, int W, int gw, unsigned int *L, int lane) {
  for_centre_words<BLOCK>(cpl, crows, W, [&](int r, int w, unsigned long long cw, int tw) {
    const unsigned int i = (unsigned int)(r * gw + w * 64 + lane);
    unsigned int p = 0u;
    bool todo = false;
    if ((cw >> lane) & 1ull) {
      p = find_root(L, i);
      todo = p != i;
      if (todo) __hip_atomic_store(&L[i], p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    unsigned long long b;
    while ((b = __ballot(todo)) != 0ull) {
      const int leader = __ffsll((long long)b) - 1;
      const unsigned int p0 = (unsigned int)__shfl((int)p, leader);
      const bool same = todo && p == p0;
      const unsigned long long sb = __ballot(same);
      if (lane == leader) atomicAdd(&L[p0], (unsigned int)__popcll(sb));
      todo = todo && !same;
    }
  });
}

// winner: the number of roots into total[1], and the largest (cells, smallest root index first) into the u64 at total[2]
template <int BLOCK>
__device__ __forceinline__ void winner(const unsigned long long *cpl, int crows, int W, int gw, const unsigned int *L,
                                       unsigned int *total, int lane) {
  unsigned long long *best = reinterpret_cast<unsigned long long *>(total + 2);
  for_centre_words<BLOCK>(cpl, crows, W, [&](int r, int w, unsigned long long cw, int tw) {
    const unsigned int i = (unsigned int)(r * gw + w * 64 + lane);
    unsigned int v = 0u;
    if ((cw >> lane) & 1ull) v = L[i];
    const bool root = (v & kRoot) != 0u;
    const unsigned long long rb = __ballot(root);
    if (root) {
      if (lane == __ffsll((long long)rb) - 1) atomicAdd(&total[1], (unsigned int)__popcll(rb));
      atomicMax(best, ((unsigned long long)((v & ~kRoot) + 1u) << 32) | (unsigned long long)(0xffffffffu - i));
    }
  });
}

// box: LDS min / max over the winner's cells (its root `win`, and every cell whose label is the root)
template <int BLOCK>
__device__ __forceinline__ void box(const unsigned long long *cpl, int crows, int W, int gw, const unsigned int *L,
                                    unsigned int *total, unsigned int win, int lane) {
  for_centre_words<BLOCK>(cpl, crows, W, [&](int r, int w, unsigned long long cw, int tw) {
    const unsigned int i = (unsigned int)(r * gw + w * 64 + lane);
    bool mine = false;
    if ((cw >> lane) & 1ull) mine = i == win || L[i] == win;
    const unsigned long long mb = __ballot(mine);
    if (mine && lane == __ffsll((long long)mb) - 1) {
      atomicMin(&total[4], (unsigned int)(w * 64 + lane));
      atomicMax(&total[6], (unsigned int)(w * 64 + 63 - __clzll((long long)mb)));
      atomicMin(&total[5], (unsigned int)r);
      atomicMax(&total[7], (unsigned int)r);
    }
  });
}

}  // namespace blob_label
}  // namespace mtgpu
