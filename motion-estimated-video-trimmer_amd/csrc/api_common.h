// api_common.h — what the entry points of mtgpu_api.hip share: the layout of a host form's staging block, the
// profiled launch, the work-list scratch guard, the launch-struct header, the host forms' staging and the rungs of the
// argument ladders.  Internal, and included by mtgpu_api.hip ALONE, behind its mtgpu_ctx and the scratch ring (the
// helpers below the layout use both).
//
// An entry point's rungs — which check comes first, and the text it answers with — are ABI: callers see them through
// (rc, mtgpu_last_error()).  The helpers here only spell a rung once; every entry point still calls them in its own
// order, and tests/test_api_arg_rungs_host.py pins that order.  Change it only on purpose.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mtgpu {

// ---- the layout of a staging block.  No HIP and no context: tests/cpp/stage_layout_check.cpp includes this part alone
// (MTGPU_STAGE_LAYOUT_ONLY) and holds it to the formulas the host forms wrote out by hand before.
//
// The extra inputs of a host form and then its outputs lie in one device block, every slot at the next multiple of 256
// bytes.  A slot that is not present takes no room; a present slot of 0 bytes takes none either.
constexpr int kStageMaxSlots = 10;      // the heading scan's host form: two inputs, seven outputs
constexpr size_t kNoSlot = ~(size_t)0;
struct StageSlot { size_t bytes; bool present; };
inline size_t stage_up(size_t v) { return (v + 255u) & ~(size_t)255u; }
// off[i]: where slot i begins, kNoSlot when it is not present.  Returns the bytes to reserve: the 256-byte step behind
// the last slot, or, with exact_tail, its last byte (the plain scan and the sweep size d_flags so; mtgpu_get_stats shows it).
inline size_t stage_layout(const StageSlot *s, int n, bool exact_tail, size_t *off) {
  size_t at = 0, end = 0;
  for (int i = 0; i < n; ++i) {
    off[i] = s[i].present ? at : kNoSlot;
    if (!s[i].present) continue;
    end = at + s[i].bytes;
    at += stage_up(s[i].bytes);
  }
  return exact_tail ? end : at;
}

}  // namespace mtgpu

#ifndef MTGPU_STAGE_LAYOUT_ONLY
#include <initializer_list>

namespace {

#define MT_TRY(expr)                    \
  do {                                  \
    const int _rc = (expr);             \
    if (_rc != MT_OK) return _rc;       \
  } while (0)

// ---------------------------------------------------------------- the launch tail

// One launch on `st`, inside the event triple {before planning, planned, scanned} of mtgpu_profile_enable when that is
// on: t[0], the launcher (which records L.ev_planned = t[1] behind its planning kernels), t[2]; the triple counts only
// when all of it was queued.  pf.mu is held across a profiled launch.
template <class Launch>
int profiled_launch(mtgpu_ctx *c, hipStream_t st, Launch &L, hipError_t (*launcher)(const Launch &), const char *what) {
  mtgpu_ctx::Profile &pf = c->prof;
  std::unique_lock<std::mutex> lock(pf.mu, std::defer_lock);
  hipEvent_t *t = nullptr;
  hipError_t e = hipSuccess;
  if (pf.on.load(std::memory_order_relaxed)) {
    lock.lock();
    if (pf.created && pf.count == mtgpu_ctx::Profile::kRing) e = pf.drain_one();
    if (e == hipSuccess && pf.created) t = pf.ev[(pf.tail + pf.count) % mtgpu_ctx::Profile::kRing];
  }
  if (t) e = hipEventRecord(t[0], st);
  L.ev_planned = t ? t[1] : nullptr;
  if (e == hipSuccess) e = launcher(L);
  if (t && e == hipSuccess) e = hipEventRecord(t[2], st);
  if (t && e == hipSuccess) ++pf.count;
  return e == hipSuccess ? MT_OK : hip_fail(e, what);
}

// The block a launch keeps its work list in: the caller's own (`own`: a pipe's batch, nothing comes from the ring), or
// `bytes` of the context's scratch ring for work queued on `st` (0 bytes: nothing, p stays null).  The ring slot goes
// back when the guard leaves scope, i.e. behind the last launch the function queued, on every way out of it.
struct PlanWs {
  mtgpu_ctx *c;
  hipStream_t st;
  int slot = -1;
  void *p;
  int rc = MT_OK;          // of scratch_acquire: look at it before p
  PlanWs(mtgpu_ctx *c_, hipStream_t st_, void *own, size_t bytes) : c(c_), st(st_), p(own) {
    if (!own && bytes) rc = scratch_acquire(c, bytes, st, &slot, &p);
  }
  ~PlanWs() { if (slot >= 0) scratch_release(c, slot, st); }
  PlanWs(const PlanWs &) = delete;
  PlanWs &operator=(const PlanWs &) = delete;
};

// ---------------------------------------------------------------- the launch structs

// max(1, analysed rows): what the LDS layouts are sized for (ScanK::y_lo / y_hi, make_plan)
int analysed_rows(const mt_scan_params &p) {
  const int y_lo = p.vertical_margin;
  int y_hi = p.grid_h - p.vertical_margin;
  if (y_hi < y_lo) y_hi = y_lo;
  return (y_hi - y_lo) < 1 ? 1 : (y_hi - y_lo);
}

// The header every launch struct shares (mtgpu::BatchLaunch): the batch, the device limits, no scratch and no event yet.
void fill_batch(mtgpu::BatchLaunch &L, const mtgpu_ctx *c, const void *d_rec, int rec_bytes, uint64_t n_records, uint64_t rebase,
                const uint64_t *d_off, const uint8_t *d_sd, uint32_t n_frames, int lds_bytes, hipStream_t st) {
  L.mv = static_cast<const unsigned char *>(d_rec);
  L.n_records = n_records;
  L.rebase = rebase;
  L.frame_off = reinterpret_cast<const unsigned long long *>(d_off);
  L.has_sd = d_sd;
  L.n_frames = n_frames;
  L.rec_bytes = rec_bytes;
  L.lds_bytes = lds_bytes;
  L.lds_max = c->lds_max;
  L.device = c->device;
  L.plan_ws = nullptr;
  L.stream = st;
  L.ev_planned = nullptr;
}

// A zeroed kernel parameter block with the grid of the context's ScanK.  Host code: the blocks themselves are kernel
// arguments and keep their layouts.
template <class K>
void fill_grid(K &k, const mtgpu::ScanK &from) {
  std::memset(&k, 0, sizeof k);
  k.shift = from.shift; k.gw = from.gw; k.gh = from.gh; k.y_lo = from.y_lo; k.y_hi = from.y_hi; k.W = from.W;
}
// ... and, for the one-tile kernels (ActK, ZoneK, BlobK, GmcK, GmcBlobK, DirK), the vote's settings, R and the tile.
template <class K>
void fill_tile(K &k, const mtgpu::ScanK &from, size_t (*tile_words)(int gw, int R)) {
  fill_grid(k, from);
  k.thr = from.thr; k.vec_need = from.vec_need;
  k.R = (k.y_hi - k.y_lo) < 1 ? 1 : (k.y_hi - k.y_lo);
  k.tile_words = (int)tile_words(k.gw, k.R);
}

// Has the context's grid a form of this kind (plan_fn names the grid when not)?  No HIP call.
template <class Plan>
int plan_ok(const mtgpu_ctx *c, int (*plan_fn)(const mt_scan_params &, int, Plan *)) {
  Plan pl;
  return plan_fn(c->params, c->lds_max, &pl);
}

// The body of an mtgpu_*_preview.
template <class Plan>
int preview(const mt_scan_params *p, int lds_bytes_per_workgroup, Plan *out, int (*plan_fn)(const mt_scan_params &, int, Plan *)) {
  if (!out) return fail(MT_ERR_INVALID, "out is NULL");
  MT_TRY(validate_params(p));
  if (lds_bytes_per_workgroup < 1024) return fail(MT_ERR_INVALID, "LDS size out of range");
  Plan pl;
  MT_TRY(plan_fn(*p, lds_bytes_per_workgroup, &pl));
  *out = pl;
  return MT_OK;
}

// The work-list block a pipe hands to a ctx_launch_* doorway.  what: "masked", "blob", ...
int check_pipe_ws(const char *what, const void *plan_ws, size_t bytes, uint32_t n_frames) {
  if (!plan_ws || ((uintptr_t)plan_ws & 255u) != 0u || bytes < mtgpu::plan_scratch_bytes(n_frames))
    return fail(MT_ERR_INVALID, "%s pipe scan: the batch's work-list block is missing, misaligned or too small", what);
  return MT_OK;
}

// ---------------------------------------------------------------- the rungs of the argument ladders
// `d`: "d_" in a device entry point, "" in a host one (the names in the texts are the header's parameter names).

struct NamedPtr { const char *name; const void *p; };
struct AlignedPtr { const char *name; const void *p; unsigned align; };

int check_rec_bytes(int rec_bytes) {
  if (rec_bytes != MT_MV_BYTES && rec_bytes != MT_COMPACT_BYTES)
    return fail(MT_ERR_INVALID, "rec_bytes must be %d (mt_mv) or %d (mt_mv_compact), not %d", MT_MV_BYTES, MT_COMPACT_BYTES, rec_bytes);
  return MT_OK;
}

// The records' alignment: 8 bytes for compact ones, 4 for any.  The 4-byte rung names the argument itself, "d_rec" in
// the device entry points and "mv" in the host ones.
int check_rec(const char *d, int rec_bytes, const void *rec) {
  if (rec_bytes == MT_COMPACT_BYTES && ((uintptr_t)rec & 7u) != 0)
    return fail(MT_ERR_INVALID, "%srec: compact records must be 8-byte aligned", d);
  if (((uintptr_t)rec & 3u) != 0) return fail(MT_ERR_INVALID, "%s must be 4-byte aligned", d[0] ? "d_rec" : "mv");
  return MT_OK;
}

// "a and b are both NULL" / "a, b and c are all NULL"
int check_any_output(const char *d, std::initializer_list<NamedPtr> outs) {
  char names[256];
  size_t at = 0, i = 0;
  for (const NamedPtr &o : outs) {
    if (o.p) return MT_OK;
    const char *sep = i == 0 ? "" : (i + 1 == outs.size() ? " and " : ", ");
    const int n = snprintf(names + at, sizeof names - at, "%s%s%s", sep, d, o.name);
    if (n > 0) at = std::min(at + (size_t)n, sizeof names - 1);
    ++i;
  }
  return fail(MT_ERR_INVALID, "%s are %s NULL", names, outs.size() == 2 ? "both" : "all");
}

// the first of them that is not aligned (a null pointer is)
int check_aligned(const char *d, std::initializer_list<AlignedPtr> ptrs) {
  for (const AlignedPtr &a : ptrs)
    if (((uintptr_t)a.p & (uintptr_t)(a.align - 1u)) != 0) return fail(MT_ERR_INVALID, "%s%s must be %u-byte aligned", d, a.name, a.align);
  return MT_OK;
}

// A keep mask comes with its stream table or not at all (blobs, gmc_blobs).  The masked scan REQUIRES both and the
// direction scan words the same rule about `allows`: their rungs stand in their own ladders.
int check_stream_table(const char *d, const void *stream_off, uint32_t n_streams, const void *keep) {
  if (keep && !stream_off) return fail(MT_ERR_INVALID, "%sstream_off is NULL with %skeep given", d, d);
  if (keep && n_streams == 0) return fail(MT_ERR_INVALID, "n_streams is 0 with %skeep given", d);
  if (!keep && stream_off) return fail(MT_ERR_INVALID, "%skeep is NULL with %sstream_off given", d, d);
  if (!keep && n_streams != 0) return fail(MT_ERR_INVALID, "%skeep is NULL with n_streams %u", d, n_streams);
  return MT_OK;
}

// host forms: off[0 .. n] non-decreasing.  ("frame_off", "frame") / ("stream_off", "stream")
int check_monotonic(const char *name, const char *unit, const uint64_t *off, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return fail(MT_ERR_INVALID, "%s not monotonic at %s %u", name, unit, i);
  return MT_OK;
}
// host forms: the streams are non-decreasing and end at the batch's last frame
int check_stream_off(const uint64_t *stream_off, uint32_t n_streams, uint32_t n_frames) {
  MT_TRY(check_monotonic("stream_off", "stream", stream_off, n_streams));
  if (stream_off[n_streams] != (uint64_t)n_frames)
    return fail(MT_ERR_INVALID, "stream_off[%u] is %llu, not n_frames %u", n_streams, (unsigned long long)stream_off[n_streams], n_frames);
  return MT_OK;
}

// host forms: the records the offsets span are [*r_begin, *r_end) of mv
int check_window(const mt_mv *mv, const uint64_t *frame_off, uint32_t n_frames, uint64_t *r_begin, uint64_t *r_end) {
  *r_begin = n_frames ? frame_off[0] : 0;
  *r_end = n_frames ? frame_off[n_frames] : 0;
  if (*r_end - *r_begin > 0 && !mv) return fail(MT_ERR_INVALID, "mv is NULL with records present");
  return MT_OK;
}

// Is p memory of the context's device?
bool on_ctx_device(const mtgpu_ctx *c, const void *p) {
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof at);
  const hipError_t qe = hipPointerGetAttributes(&at, p);
  if (qe != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeDevice && at.device == c->device;
}
// device entry points: the first of the given arrays (null: not given) that is not memory of the context's device
int check_on_device(const mtgpu_ctx *c, std::initializer_list<NamedPtr> ptrs, const char *why = "") {
  for (const NamedPtr &a : ptrs)
    if (a.p && !on_ctx_device(c, a.p)) return fail(MT_ERR_INVALID, "%s is not memory of device %d%s", a.name, c->device, why);
  return MT_OK;
}

// ---------------------------------------------------------------- the host forms' staging

// A host batch on its way through the context's staging buffers: the records the offsets span go to d_mv, the offsets
// to d_off, has_sd to d_sd, and the form's extra inputs and its outputs to the slots of ONE block (`block`: d_misc, or
// d_flags for the plain scan and the sweep; stage_layout).  Declare the slots with in() / out() in the order of the
// layout, upload(), run the form's *_on with the device pointers (rebased offsets: frame f's records live at
// d_mv() + (frame_off[f] - r_begin) * 40), download().  c->mu is held from construction on, and the object synchronises
// the context's stream when it leaves scope once anything was queued: the copies read and write CALLER memory.
struct Staged {
  mtgpu_ctx *c;
  DevBuf &block;
  const bool exact_tail;
  const mt_mv *mv;
  const uint64_t r_begin, r_end;
  const uint64_t *frame_off;
  const uint8_t *has_sd;               // staged only when the batch has frames
  const uint32_t n_frames;
  hipStream_t st;
  std::lock_guard<std::mutex> lock;
  bool queued = false;
  int n = 0, n_in = 0;
  void *host[mtgpu::kStageMaxSlots];
  mtgpu::StageSlot slot[mtgpu::kStageMaxSlots];
  size_t off[mtgpu::kStageMaxSlots];

  Staged(mtgpu_ctx *c_, DevBuf &block_, bool exact_tail_, const mt_mv *mv_, uint64_t r_begin_, uint64_t r_end_, const uint64_t *frame_off_,
         const uint8_t *has_sd_, uint32_t n_frames_)
      : c(c_), block(block_), exact_tail(exact_tail_), mv(mv_), r_begin(r_begin_), r_end(r_end_), frame_off(frame_off_),
        has_sd(n_frames_ ? has_sd_ : nullptr), n_frames(n_frames_), st(c_->stream), lock(c_->mu) {}
  ~Staged() { if (queued) (void)hipStreamSynchronize(st); }

  // an extra input (null: not given — no room, no copy, a null device pointer); all of them before the first out()
  int in(const void *p, size_t bytes) {
    host[n] = const_cast<void *>(p);
    slot[n] = {p ? bytes : 0u, true};
    n_in = n + 1;
    return n++;
  }
  // an output (null: not asked for — a null device pointer, and no room unless `always`)
  int out(void *p, size_t bytes, bool always = false) {
    host[n] = p;
    slot[n] = {bytes, p != nullptr || always};
    return n++;
  }
  template <class T>
  T *at(int i) const { return host[i] ? reinterpret_cast<T *>(static_cast<unsigned char *>(block.p) + off[i]) : nullptr; }
  const void *d_mv() const { return c->d_mv.p; }
  const uint64_t *d_off() const { return static_cast<const uint64_t *>(c->d_off.p); }
  const uint8_t *d_sd() const { return has_sd ? static_cast<const uint8_t *>(c->d_sd.p) : nullptr; }

  int upload() {
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t n_records = r_end - r_begin;
    MT_TRY(c->d_mv.reserve((size_t)n_records * MT_MV_BYTES + 16));
    MT_TRY(c->d_off.reserve(sizeof(uint64_t) * ((size_t)n_frames + 1)));
    MT_TRY(block.reserve(mtgpu::stage_layout(slot, n, exact_tail, off)));
    if (has_sd) MT_TRY(c->d_sd.reserve(n_frames));
    queued = true;
    if (n_records)
      HIP_TRY(hipMemcpyAsync(c->d_mv.p, mv + r_begin, (size_t)n_records * MT_MV_BYTES, hipMemcpyHostToDevice, st));
    if (n_frames) HIP_TRY(hipMemcpyAsync(c->d_off.p, frame_off, sizeof(uint64_t) * ((size_t)n_frames + 1), hipMemcpyHostToDevice, st));
    if (has_sd) HIP_TRY(hipMemcpyAsync(c->d_sd.p, has_sd, n_frames, hipMemcpyHostToDevice, st));
    for (int i = 0; i < n_in; ++i)
      if (slot[i].bytes) HIP_TRY(hipMemcpyAsync(at<void>(i), host[i], slot[i].bytes, hipMemcpyHostToDevice, st));
    return MT_OK;
  }
  // the outputs that were asked for, in their order, and the wait for them
  int download() {
    for (int i = n_in; i < n; ++i)
      if (host[i]) HIP_TRY(hipMemcpyAsync(host[i], at<void>(i), slot[i].bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MT_OK;
  }
};

}  // namespace
#endif  // MTGPU_STAGE_LAYOUT_ONLY
