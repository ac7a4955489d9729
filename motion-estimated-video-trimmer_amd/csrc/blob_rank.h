// blob_rank.h — what the object scan (objects_kernels.hip) adds behind the labelling of blob_label.h: a count over the
// roots (inside the first ranking round), the K largest blobs in order, and the boxes of all of them in one pass.  The conventions are blob_label.h's:
// `__device__ __forceinline__` passes over for_centre_words, a wave per 64-cell word, lane = bit, no barrier inside a
// pass, every trip count depends on the wave alone; the caller puts a workgroup barrier where a pass reads what another
// wrote.  The passes read the labels as flatten leaves them: a root holds kRoot | (cells - 1) and is the smallest cell
// index of its blob, every other centre holds its root.
//
//   total   8 u32          [0] centres, [1] blobs, [2] blobs of at least `need` cells; [3..7] unused here
//   keys    k u64          keys[j] = cells << 32 | (0xFFFFFFFF - root) of the blob of rank j, 0: no such blob.  The
//                          winner key of blob_label::winner; keys are distinct, since roots are
//   boxes   k x 4 u32      min x, min r, max x, max r of rank j ([0], [1] start at 0xffffffff, the rest at 0)
// keys and boxes are the ranking table of objects_kernels.h (objects_lds_bytes), behind `total`.
// Internal; included after blob_label.h; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blob_label.h"

namespace mtgpu {
namespace blob_rank {

__device__ __forceinline__ unsigned long long key_of(unsigned int root_word, unsigned int i) {
  return ((unsigned long long)((root_word & ~blob_label::kRoot) + 1u) << 32) | (unsigned long long)(0xffffffffu - i);
}

// One round of the ranking: the largest key strictly below `below` into *slot (0 before the round).  Round 0 takes
// below = ~0, round j the key round j - 1 found; the caller's barrier stands between two rounds.  Keys are distinct, so
// what a round finds does not depend on the order of the atomics.
// COUNT (round 0, which meets every root anyway): also the count over the roots — the blobs into total[1] and those of
// at least `need` cells into total[2], one LDS add per wave and word for each (none for a zero).  A pass of its own
// would read the centre words and the labels once more for two ballots.
template <int BLOCK, bool COUNT>
__device__ __forceinline__ void rank_round(const unsigned long long *cpl, int crows, int W, int gw, const unsigned int *L,
                                           unsigned long long *slot, unsigned long long below, unsigned int *total,
                                           unsigned int need, int lane) {
  blob_label::for_centre_words<BLOCK>(cpl, crows, W, [&](int r, int w, unsigned long long cw, int tw) {
    const unsigned int i = (unsigned int)(r * gw + w * 64 + lane);
    unsigned int v = 0u;
    if ((cw >> lane) & 1ull) v = L[i];
    const bool root = (v & blob_label::kRoot) != 0u;
    if constexpr (COUNT) {
      const unsigned long long rb = __ballot(root);
      const unsigned long long ob = __ballot(root && (v & ~blob_label::kRoot) + 1u >= need);
      if (lane == 0) {
        if (rb) atomicAdd(&total[1], (unsigned int)__popcll(rb));
        if (ob) atomicAdd(&total[2], (unsigned int)__popcll(ob));
      }
    }
    if (root) {
      const unsigned long long key = key_of(v, i);
      if (key < below) atomicMax(slot, key);
    }
  });
}

// boxes: ONE pass for all `n` listed blobs (keys[0 .. n) in descending order, n >= 1).  A cell's blob is listed iff its
// key is at least keys[n - 1]; its rank is the number of larger keys.  One set of four LDS min / max per (wave, distinct
// listed root), by the ballot loop of blob_label::flatten; cells of unlisted blobs add nothing.
template <int BLOCK>
__device__ __forceinline__ void boxes(const unsigned long long *cpl, int crows, int W, int gw, const unsigned int *L,
                                      const unsigned long long *keys, unsigned int *box, int n, int lane) {
  const unsigned long long least = keys[n - 1];
  blob_label::for_centre_words<BLOCK>(cpl, crows, W, [&](int r, int w, unsigned long long cw, int tw) {
    const unsigned int i = (unsigned int)(r * gw + w * 64 + lane);
    unsigned int p = 0u;
    unsigned long long key = 0ull;
    if ((cw >> lane) & 1ull) {
      const unsigned int v = L[i];
      p = (v & blob_label::kRoot) ? i : v;
      key = key_of((v & blob_label::kRoot) ? v : L[p], p);
    }
    bool todo = key >= least;                     // a cell that is no centre has key 0 < least
    unsigned long long b;
    while ((b = __ballot(todo)) != 0ull) {
      const int leader = __ffsll((long long)b) - 1;
      const unsigned int p0 = (unsigned int)__shfl((int)p, leader);
      const bool same = todo && p == p0;
      const unsigned long long sb = __ballot(same);
      if (lane == leader) {
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += keys[j] > key ? 1 : 0;        // < n: key is one of keys[0 .. n)
        unsigned int *bx = box + 4 * rank;
        atomicMin(&bx[0], (unsigned int)(w * 64 + lane));
        atomicMax(&bx[2], (unsigned int)(w * 64 + 63 - __clzll((long long)sb)));
        atomicMin(&bx[1], (unsigned int)r);
        atomicMax(&bx[3], (unsigned int)r);
      }
      todo = todo && !same;
    }
  });
}

}  // namespace blob_rank
}  // namespace mtgpu
