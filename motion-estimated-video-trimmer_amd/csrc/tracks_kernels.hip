// tracks_kernels.hip — gfx950 kernels for object tracks (include/mtgpu_tracks.h): per stream, which entry of the previous
// motion frame's object list each listed object continues (pred), how long it has existed (age), which track it belongs
// to (id) and how deep that track's tree gets (len); per frame the longest track among its objects.
//
// Three kernels, queued in this order on one stream:
//
//   tracks_clear_kernel    parallel over the list entries: zeroes the depth table (work[0 .. n_frames * k)) and writes the
//                          empty values to the entries of frames outside [stream_off[0], stream_off[n_streams]).
//   tracks_streams_kernel  one 256-lane workgroup per stream, grid stride over the streams.  The workgroup walks the
//                          stream forwards in tiles of 256 frames.  Sixteen lanes — a GROUP — share a frame, lane j of a
//                          group holds entry j of the list; a group takes sixteen consecutive frames of the tile.
//       (a) previous M frame   persistence's first scan, one frame per lane: M frame i is (i + 1, 0), Q is (0, 1), T is
//                              (0, 0); a . b = b.mark ? b : (a.mark, a.count + b.count).  The exclusive prefix of an M
//                              frame is (p + 1 or 0, q).  The frames of a group were scanned by the group's own lanes,
//                              so a width-16 shuffle hands each frame's prefix to its sixteen lanes.  This unit carries
//                              its own copy of that twenty-line scan: persist_kernels.* stay as they are.
//       (b) links              state-free, every group at once.  Lane j loads entry j of f and entry j of p(f) — from the
//                              input list, p(f) may lie in an earlier tile — and sixteen width-16 shuffles of the
//                              previous boxes find the lowest linked present i.  An absent previous entry shuffles the
//                              all-0xFFFF box, which links to nothing.
//       (c) ages and ids       a scan over frames whose element is a MAP spread over the sixteen lanes of a group:
//                              (src, add, rid) per entry j, meaning age_out[j] = (src none ? 0 : age_in[src]) + add and
//                              id_out[j] = src none ? rid : id_in[src].  An M frame's element is (pred, 1, f*k + j), or
//                              (none, 0, none) for an absent entry; T and Q frames and padding are the identity
//                              (j, 0, -).  A before B composes to
//                                  B.src none ? B : (A.src[B.src], A.add[B.src] + B.add, A.rid[B.src])
//                              — three width-16 shuffles, associative.  The levels are persistence's: a group folds its
//                              sixteen frames (pass 1), the sixteen group totals meet in LDS behind ONE barrier, every
//                              group applies the totals in front of it to the state behind the previous tile, and then
//                              walks its frames again with that state (pass 2).  A stream starts from the empty state,
//                              so what is carried from tile to tile is a state (age, id per entry), not a map.
//       (d) store              pred, age and id (the ids go to work[n_frames * k ..) when id is null), and a global
//                              atomicMax(depth[id], age).  A lane that holds the same id in consecutive frames of its
//                              group keeps the maximum in a register and issues ONE atomic for them: a maximum is
//                              order-free, so this cannot be observed.  Vector stores and vector atomics only.
//   tracks_finish_kernel   parallel over the frames, sixteen lanes a frame: len = depth[id], track[f] as a 16-lane
//                          maximum, flags_out.
//
// No scratch ring, no allocation, static LDS only.  Every barrier sits in control flow that depends on the stream's
// bounds alone, which the whole workgroup reads alike; every shuffle sits outside divergent branches.  stream_off
// entries are clamped to n_frames before anything is addressed, so offsets that lie (the device entry point trusts them)
// cannot reach outside the caller's arrays; a previous M frame lies inside its stream by construction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tracks_kernels.h"

#if !defined(__HIP_DEVICE_COMPILE__) || defined(__gfx950__)
#else
#error "tracks_kernels.hip is written for gfx950 only (wave64)"
#endif

namespace mtgpu {

namespace {

constexpr int TB = kTracksBlock;
constexpr int TG = kTracksGroup;
constexpr int TW = TB / 64;            // waves
constexpr int NG = TB / TG;            // groups, and the frames a group takes per tile
static_assert(TB % 64 == 0 && TG == 16 && NG == TG && kTracksTile == NG * TG, "sixteen groups of sixteen lanes, one frame per lane in the first scan");

constexpr unsigned int NONE = 0xFFu;           // no predecessor / no source
constexpr unsigned int NO_ID = 0xFFFFFFFFu;

struct St { unsigned int mark, count; };

__device__ __forceinline__ St comb(St a, St b) {
  St r;
  r.mark = b.mark ? b.mark : a.mark;
  r.count = b.mark ? b.count : a.count + b.count;
  return r;
}

// One element per lane, lane l at scan position l.  Returns the exclusive prefix of the lane with `carry` (everything
// scanned in earlier tiles) in front; carry becomes the prefix behind the tile.  ws: TW states in LDS; the barrier of
// step (c) separates this call's reads from the next call's writes.
__device__ __forceinline__ St tile_scan(St x, St &carry, St *ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  St t = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    St o;
    o.mark = __shfl_up(t.mark, d);
    o.count = __shfl_up(t.count, d);
    if (lane >= d) t = comb(o, t);
  }
  St e;
  e.mark = __shfl_up(t.mark, 1);
  e.count = __shfl_up(t.count, 1);
  if (lane == 0) e.mark = e.count = 0u;
  if (lane == 63) ws[wave] = t;
  __syncthreads();
  St pre = carry, tot = carry;
#pragma unroll
  for (int w = 0; w < TW; ++w) {
    const St s = ws[w];
    tot = comb(tot, s);
    if (w < wave) pre = comb(pre, s);
  }
  carry = tot;
  return comb(pre, e);
}

// include/mtgpu_tracks.h: linked(A, B) on the packed bounds (x0 | y0 << 16, x1 | y1 << 16); 32-bit arithmetic, reach <= 65535
__device__ __forceinline__ bool linked(unsigned int a0, unsigned int a1, unsigned int b0, unsigned int b1, unsigned int reach) {
  if ((a0 & a1) == 0xFFFFFFFFu || (b0 & b1) == 0xFFFFFFFFu) return false;
  const unsigned int ax0 = a0 & 0xFFFFu, ay0 = a0 >> 16, ax1 = a1 & 0xFFFFu, ay1 = a1 >> 16;
  const unsigned int bx0 = b0 & 0xFFFFu, by0 = b0 >> 16, bx1 = b1 & 0xFFFFu, by1 = b1 >> 16;
  return bx0 <= ax1 + reach && ax0 <= bx1 + reach && by0 <= ay1 + reach && ay0 <= by1 + reach;
}

}  // namespace

// The depth table starts at zero; entries of frames outside [stream_off[0], stream_off[n_streams]) read the empty values.
__global__ __launch_bounds__(TB) void tracks_clear_kernel(const unsigned long long *__restrict__ stream_off, unsigned int n_streams,
                                                          unsigned int n_frames, unsigned int k, unsigned int *__restrict__ depth,
                                                          unsigned int *__restrict__ idbuf, unsigned char *__restrict__ pred,
                                                          unsigned int *__restrict__ age) {
  unsigned long long lo = stream_off[0], hi = stream_off[n_streams];
  if (lo > n_frames) lo = n_frames;
  if (hi > n_frames) hi = n_frames;
  if (hi < lo) hi = lo;
  const unsigned int total = n_frames * k;                 // < 0xFFFFFFFF
  const unsigned long long step = (unsigned long long)gridDim.x * TB;
  for (unsigned long long e = (unsigned long long)blockIdx.x * TB + threadIdx.x; e < total; e += step) {
    if (depth) depth[e] = 0u;
    const unsigned int f = (unsigned int)e / k;
    if (f >= lo && f < hi) continue;
    if (pred) pred[e] = (unsigned char)NONE;
    if (age) age[e] = 0u;
    idbuf[e] = NO_ID;
  }
}

__global__ __launch_bounds__(TB) void tracks_streams_kernel(
    const unsigned char *__restrict__ flags, const unsigned char *__restrict__ has_sd, const uint4 *__restrict__ list, unsigned int k,
    unsigned int n_frames, const unsigned long long *__restrict__ stream_off, unsigned int n_streams, unsigned int need_cells,
    unsigned int max_dropout, unsigned int reach, unsigned int *__restrict__ depth, unsigned int *__restrict__ idbuf,
    unsigned char *__restrict__ pred, unsigned int *__restrict__ age) {
  __shared__ St ws[TW];
  __shared__ unsigned int t_src[NG][TG], t_add[NG][TG], t_rid[NG][TG];
  const unsigned int j = threadIdx.x & (TG - 1), g = threadIdx.x / TG;
  const bool lane_on = j < k;

  for (unsigned int s = blockIdx.x; s < n_streams; s += gridDim.x) {
    unsigned long long b = stream_off[s], e = stream_off[s + 1];
    if (b > n_frames) b = n_frames;
    if (e > n_frames) e = n_frames;
    if (e < b) e = b;
    const unsigned long long len = e - b;                // < 2^32
    const unsigned long long tiles = (len + TB - 1) / TB;

    St carry = {0u, 0u};
    unsigned int c_age = 0u, c_id = NO_ID;               // entry j behind the previous tile: the stream starts empty
    for (unsigned long long t = 0; t < tiles; ++t) {
      // ---- (a) one frame per lane: its class, its previous M frame and the Q frames since
      const unsigned long long mine = t * TB + threadIdx.x;
      St x = {0u, 0u};
      unsigned int my_m = 0u;
      if (mine < len) {
        if (flags[b + mine] != 0) {
          my_m = 1u;
          x.mark = (unsigned int)mine + 1u;
        } else if (!has_sd || has_sd[b + mine] != 0) {
          x.count = 1u;                                    // Q; a T frame stays (0, 0)
        }
      }
      const St before = tile_scan(x, carry, ws);           // (p + 1 or 0, Q frames since p)

      // ---- (b) links and (c) pass 1: the group's sixteen frames folded into one map
      const unsigned long long i0 = t * TB + (unsigned long long)g * NG;   // the group's first frame, relative to the stream
      unsigned int r_src = j, r_add = 0u, r_rid = NO_ID;
      unsigned long long preds = 0ull;                     // four bits a frame: pred & 15
      unsigned int nonem = 0u, presm = 0u;                 // one bit a frame: pred is none / the entry is present
#pragma unroll 1
      for (int fi = 0; fi < NG; ++fi) {
        const bool is_m = __shfl(my_m, fi, TG) != 0u;
        const unsigned int pm = __shfl(before.mark, fi, TG), q = __shfl(before.count, fi, TG);
        const unsigned long long f = b + i0 + fi;          // an M frame lies inside the stream
        unsigned int cells = 0u, c0 = 0xFFFFFFFFu, c1 = 0xFFFFFFFFu, p0 = 0xFFFFFFFFu, p1 = 0xFFFFFFFFu;
        if (is_m && lane_on) {
          const uint4 cur = list[f * k + j];
          cells = cur.x;
          c0 = cur.z;
          c1 = cur.w;
          if (pm != 0u && q <= max_dropout) {
            const uint4 prv = list[(b + (pm - 1u)) * k + j];
            if (prv.x >= need_cells) {                     // an absent entry keeps the box that links to nothing
              p0 = prv.z;
              p1 = prv.w;
            }
          }
        }
        const bool pres = is_m && lane_on && cells >= need_cells;
        unsigned int pr = NONE;
#pragma unroll
        for (int i = TG - 1; i >= 0; --i) {                // descending: the lowest linked i is written last
          const unsigned int a0 = __shfl(p0, i, TG), a1 = __shfl(p1, i, TG);
          if (linked(a0, a1, c0, c1, reach)) pr = (unsigned int)i;
        }
        if (!pres) pr = NONE;
        const unsigned int from = pr & (TG - 1);
        const unsigned int a_src = __shfl(r_src, from, TG), a_add = __shfl(r_add, from, TG), a_rid = __shfl(r_rid, from, TG);
        if (is_m) {
          if (pr != NONE) {
            r_src = a_src;
            r_add = a_add + 1u;
            r_rid = a_rid;
          } else {
            r_src = NONE;
            r_add = pres ? 1u : 0u;
            r_rid = pres ? (unsigned int)(f * k + j) : NO_ID;
          }
        }
        preds |= (unsigned long long)from << (4 * fi);
        nonem |= (pr == NONE ? 1u : 0u) << fi;
        presm |= (pres ? 1u : 0u) << fi;
      }
      t_src[g][j] = r_src;
      t_add[g][j] = r_add;
      t_rid[g][j] = r_rid;
      __syncthreads();

      // ---- the group totals in front of this group, applied to the state behind the previous tile
      unsigned int p_age = c_age, p_id = c_id, pre_age = c_age, pre_id = c_id;
#pragma unroll 4
      for (unsigned int w = 0; w < (unsigned int)NG; ++w) {
        if (w == g) {
          pre_age = p_age;
          pre_id = p_id;
        }
        const unsigned int ts = t_src[w][j], ta = t_add[w][j], tr = t_rid[w][j];
        const unsigned int s_age = __shfl(p_age, ts & (TG - 1), TG), s_id = __shfl(p_id, ts & (TG - 1), TG);
        p_age = ts == NONE ? ta : s_age + ta;
        p_id = ts == NONE ? tr : s_id;
      }
      c_age = p_age;
      c_id = p_id;

      // ---- (c) pass 2 and (d): the group's frames again, with the state in front of them
      unsigned int v_age = pre_age, v_id = pre_id;
      unsigned int pend_id = NO_ID, pend_age = 0u;         // the chain this lane is following: one atomic when it ends
#pragma unroll 1
      for (int fi = 0; fi < NG; ++fi) {
        const bool is_m = __shfl(my_m, fi, TG) != 0u;
        const unsigned int from = (unsigned int)(preds >> (4 * fi)) & (TG - 1);
        const unsigned int s_age = __shfl(v_age, from, TG), s_id = __shfl(v_id, from, TG);
        const unsigned long long i = i0 + fi;
        const unsigned long long at = (b + i) * k + j;     // used only where i < len and j < k: below n_frames * k
        unsigned int o_pred = NONE, o_age = 0u, o_id = NO_ID;
        if (is_m) {
          const bool pres = (presm >> fi) & 1u, none = (nonem >> fi) & 1u;
          if (!pres) {
            v_age = 0u;
            v_id = NO_ID;
          } else if (none) {
            v_age = 1u;
            v_id = (unsigned int)at;
          } else {
            v_age = s_age + 1u;
            v_id = s_id;
            o_pred = from;
          }
          o_age = v_age;
          o_id = v_id;
          if (pres && depth) {
            if (pend_id != v_id) {
              if (pend_id != NO_ID) atomicMax(&depth[pend_id], pend_age);
              pend_id = v_id;
              pend_age = v_age;
            } else if (v_age > pend_age) {
              pend_age = v_age;
            }
          }
        }
        if (i < len && lane_on) {
          if (pred) pred[at] = (unsigned char)o_pred;
          if (age) age[at] = o_age;
          idbuf[at] = o_id;
        }
      }
      if (pend_id != NO_ID) atomicMax(&depth[pend_id], pend_age);
    }
    // the next stream's first scan writes ws behind the barrier of this stream's last step (c), and t_* behind its own
    // first barrier: nothing of this stream is still being read then
  }
}

// len = depth[id]; track[f] = the largest len of the frame; flags_out.  Entries of frames outside the streams hold
// NO_ID (the clear kernel), so those frames read len 0, track 0, flags_out 0.
__global__ __launch_bounds__(TB) void tracks_finish_kernel(const unsigned char *__restrict__ flags, unsigned int k, unsigned int n_frames,
                                                           unsigned int need_track, const unsigned int *__restrict__ depth,
                                                           const unsigned int *__restrict__ idbuf, unsigned int *__restrict__ len,
                                                           unsigned int *__restrict__ track, unsigned char *__restrict__ flags_out) {
  const unsigned int j = threadIdx.x & (TG - 1), g = threadIdx.x / TG;
  const unsigned long long step = (unsigned long long)gridDim.x * NG;
  for (unsigned long long base = (unsigned long long)blockIdx.x * NG; base < n_frames; base += step) {   // uniform in the workgroup
    const unsigned long long f = base + g;
    unsigned int v = 0u;
    if (f < n_frames && j < k) {
      const unsigned int id = idbuf[f * k + j];
      v = id == NO_ID ? 0u : depth[id];
      if (len) len[f * k + j] = v;
    }
#pragma unroll
    for (int d = TG / 2; d > 0; d >>= 1) {
      const unsigned int o = __shfl_xor(v, d, TG);
      v = o > v ? o : v;
    }
    if (f < n_frames && j == 0u) {
      if (track) track[f] = v;
      if (flags_out) flags_out[f] = (flags[f] != 0 && v >= need_track) ? 1 : 0;
    }
  }
}

hipError_t launch_tracks(const TracksLaunch &L) {
  if (L.n_frames == 0 || L.n_streams == 0) return hipSuccess;
  if (!L.flags || !L.list || !L.stream_off || !L.work || L.k < 1u || L.k > (unsigned int)TG || L.need_cells == 0u || L.need_track == 0u ||
      (unsigned long long)L.n_frames * L.k >= 0xFFFFFFFFull || (!L.pred && !L.age && !L.id && !L.len && !L.track && !L.flags_out))
    return hipErrorInvalidValue;
  const unsigned int total = L.n_frames * L.k;
  const bool finish = L.len || L.track || L.flags_out;
  unsigned int *const depth = finish ? L.work : nullptr;               // nobody reads the depths otherwise
  unsigned int *const idbuf = L.id ? L.id : L.work + total;
  const unsigned int clear_blocks = (total + TB - 1u) / TB, finish_blocks = (L.n_frames + NG - 1u) / NG;
  hipLaunchKernelGGL(tracks_clear_kernel, dim3(clear_blocks < 2048u ? clear_blocks : 2048u), dim3(TB), 0, L.stream, L.stream_off, L.n_streams,
                     L.n_frames, L.k, depth, idbuf, L.pred, L.age);
  hipLaunchKernelGGL(tracks_streams_kernel, dim3(L.n_streams < 65536u ? L.n_streams : 65536u), dim3(TB), 0, L.stream, L.flags, L.has_sd,
                     reinterpret_cast<const uint4 *>(L.list), L.k, L.n_frames, L.stream_off, L.n_streams, L.need_cells, L.max_dropout, L.reach,
                     depth, idbuf, L.pred, L.age);
  if (finish)
    hipLaunchKernelGGL(tracks_finish_kernel, dim3(finish_blocks < 4096u ? finish_blocks : 4096u), dim3(TB), 0, L.stream, L.flags, L.k, L.n_frames,
                       L.need_track, depth, idbuf, L.len, L.track, L.flags_out);
  return hipGetLastError();
}

}  // namespace mtgpu
