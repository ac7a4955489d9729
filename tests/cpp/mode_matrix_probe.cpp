// mode_matrix_probe.cpp — what the host layer answers to every combination of scan modes, on one pooled GpuBackend and a
// three-frame in-memory recording (tests/host_mode_matrix.py records it into tests/golden/host_mode_matrix.json,
// tests/test_gpu_host_mode_matrix.py replays it).  Tab-separated lines:
//   grid <gw> <gh>
//   S <case>\t<ok | error text>\t<pipe state>                          scanner [full | N]: GpuMotionScanner::initialize
//   P <case>\t<rc>\t<frames_scanned>\t<error text or ->                 pipeline N: run_scan_pipeline
//   Q <x> <y>\t<ok | error text>\t<pipe state>                          pooled: the previous video ran mode x, this one asks y
// `full`: the whole product of the axes; N: every case with at most N settings off their defaults.
// A scanner case is 12 numbers: keep_centres, min_blob_cells, report_largest, gmc max_shift (-1 off), report_vector,
// gmc_blobs cells, report_gmc_blobs code, dir allow (-1 off), report_sectors, plane (0 none, 1 the grid's size, 2 a wrong
// size), keep (likewise), persist reach (-1: no persistence).
// A pipeline case is 16: keep_centres, sweep_levels, min_blob_cells, blob_sweep_levels, gmc_max_shift, gmc_vectors,
// gmc_blob_cells, gmc_blob_sweep_levels, dir_allow, dir_sectors, dir_plane, keep, min_run, reach, run_sweep_levels (levels:
// 0 none, 1 {2, 3}, 2 {1}: below CLUSTERS_NEEDED = 2), and the bits of the *_options() that are set (1 blobs 3, 2 gmc 4 with
// vectors, 4 gmc blobs 3, 8 allow 0x5B with sectors, 16 the plane, 32 min_run 3 with reach 2, 64 centres).
// The pipe state: keep=<0/1> blobs=<on>:<min>:<report> gmc=<on>:<shift>:<share>:<report> pair=<on>:<min>:<shift>:<share>:<report>
// dir=<on>:<allow>:<report> plane=<on, 9: other bytes>:<report>; "-" without a pipe.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mtgpu_host.hpp"

using namespace mtgpu_host;

class Clip : public FrameSource {   // three frames of 320 x 160, one 2 x 2 cell object moving east
  int pos_ = 0;
  std::vector<mt_mv> mv_;
 public:
  static constexpr int kW = 320, kH = 160, kFps = 25, kFrames = 3, kTb = 12800;
  Clip() : mv_((kW / 16) * (kH / 16)) {}
  int width() const override { return kW; }
  int height() const override { return kH; }
  double duration() const override { return (double)kFrames / kFps; }
  double fps() const override { return kFps; }
  double time_base() const override { return 1.0 / kTb; }
  void seek(double seconds) override {
    long f = (long)(seconds / time_base()) / (kTb / kFps);
    pos_ = (int)(f < 0 ? 0 : f >= kFrames ? kFrames - 1 : f);
  }
  bool next(Frame &fr) override {
    if (pos_ >= kFrames) return false;
    fr.pts = (int64_t)(pos_++) * (kTb / kFps);
    fr.has_side_data = true;
    for (int y = 0; y < kH / 16; ++y)
      for (int x = 0; x < kW / 16; ++x) {
        mt_mv &r = mv_[(size_t)y * (kW / 16) + x];
        r = mt_mv{};
        r.dst_x = (int16_t)(x * 16 + 8); r.dst_y = (int16_t)(y * 16 + 8);
        r.src_x = (int16_t)(r.dst_x - ((x == 5 || x == 6) && (y == 4 || y == 5) ? 6 : 0)); r.src_y = r.dst_y;
      }
    fr.mv = mv_.data();
    fr.mv_bytes = mv_.size() * sizeof(mt_mv);
    return true;
  }
};

static int g_gw = 0, g_gh = 0;
static std::vector<uint8_t> plane_of(int code) { return code ? std::vector<uint8_t>((size_t)g_gw * g_gh - (code == 2), 0x5B) : std::vector<uint8_t>(); }
static std::vector<uint64_t> keep_of(int code) { return code ? std::vector<uint64_t>((size_t)g_gh * ((g_gw + 63) / 64) + (code == 2), ~0ull) : std::vector<uint64_t>(); }

static std::string state(mtgpu_pipe *p) {
  if (!p) return "-";
  int32_t a = 0, b = 0, c = 0;
  int r = 0;
  char t[256];
  std::string s = "keep=" + std::to_string(mtgpu_pipe_has_keep(p));
  int on = mtgpu_pipe_blobs(p, &a, &r);
  std::snprintf(t, sizeof t, " blobs=%d:%d:%d", on, on ? a : 0, on ? r : 0); s += t;
  on = mtgpu_pipe_gmc(p, &a, &b, &r);
  std::snprintf(t, sizeof t, " gmc=%d:%d:%d:%d", on, on ? a : 0, on ? b : 0, on ? r : 0); s += t;
  on = mtgpu_pipe_gmc_blobs(p, &a, &b, &c, &r);
  std::snprintf(t, sizeof t, " pair=%d:%d:%d:%d:%d", on, on ? a : 0, on ? b : 0, on ? c : 0, on ? r : 0); s += t;
  on = mtgpu_pipe_dir(p, &a, &r);
  std::snprintf(t, sizeof t, " dir=%d:%d:%d", on, on ? a : 0, on ? r : 0); s += t;
  std::vector<uint8_t> back((size_t)g_gw * g_gh, 0);
  on = mtgpu_pipe_plane(p, back.data(), &r);
  std::snprintf(t, sizeof t, " plane=%d:%d", on == 1 && back != plane_of(1) ? 9 : on, on ? r : 0); s += t;
  return s;
}

// every assignment of the axes with at most `most` of them off their default (the first value); most < 0: the whole product
static void combos(const std::vector<std::vector<int>> &axes, int most, std::vector<std::vector<int>> &out) {
  std::vector<int> cur(axes.size());
  for (size_t i = 0; i < axes.size(); ++i) cur[i] = axes[i][0];
  struct Rec {
    const std::vector<std::vector<int>> &axes; int most; std::vector<std::vector<int>> &out; std::vector<int> &cur;
    void go(size_t i, int used) {
      if (i == axes.size()) { out.push_back(cur); return; }
      for (size_t k = 0; k < axes[i].size(); ++k) {
        if (k && most >= 0 && used == most) break;
        cur[i] = axes[i][k];
        go(i + 1, used + (k ? 1 : 0));
      }
      cur[i] = axes[i][0];
    }
  } rec{axes, most, out, cur};
  rec.go(0, 0);
}

static std::string join(const std::vector<int> &c) {
  std::string s;
  for (size_t i = 0; i < c.size(); ++i) s += (i ? " " : "") + std::to_string(c[i]);
  return s;
}

static bool init_scanner(Clip &clip, GpuBackend &be, const std::vector<int> &c, std::string &err) {
  GpuMotionScanner s(clip, 0, &be);
  s.keep_centres(c[0] != 0);
  s.set_min_blob_cells(c[1]); s.report_largest(c[2] != 0);
  s.set_gmc(c[3]); s.report_vector(c[4] != 0);
  s.set_gmc_blobs(c[5]); s.report_gmc_blobs(c[6]);
  s.set_dir(c[7]); s.report_sectors(c[8] != 0);
  s.set_plane(plane_of(c[9]));
  s.set_keep(keep_of(c[10]));
  s.set_persist(c[11] >= 0 ? 2 : 0, 0, c[11]);
  const bool ok = s.initialize(64, 4, 2);
  err = s.error();
  return ok;
}

static int scanner(int most) {
  Clip clip;
  GpuBackend be;
  // keep_centres outermost: the pipe's layout changes with it, and only with it
  std::vector<std::vector<int>> axes = {{0, 1}, {0, 3}, {0, 1}, {-1, 4}, {0, 1}, {0, 3}, {MT_PIPE_REPORT_CENTRES, MT_PIPE_REPORT_LARGEST, MT_PIPE_REPORT_VECTOR},
                                        {-1, 0x5B}, {0, 1}, {0, 1, 2}, {0, 1, 2}, {-1}};
  std::vector<std::vector<int>> cases;
  combos(axes, most, cases);
  // persistence with a reach: the pipe carries boxes, and only a blob scan fills them
  for (int kc : {0, 1})
    for (int reach : {2, 70000})
      for (int mb : {0, 3})
        for (int pair : {0, 3}) cases.push_back({kc, mb, 0, -1, 0, pair, MT_PIPE_REPORT_CENTRES, -1, 0, 0, 0, reach});
  for (const std::vector<int> &c : cases) {
    std::string err;
    const bool ok = init_scanner(clip, be, c, err);
    std::printf("S %s\t%s\t%s\n", join(c).c_str(), ok ? "ok" : err.c_str(), state(be.pipe()).c_str());
  }
  return 0;
}

static const std::vector<int> &levels(int code) {
  static const std::vector<int> none, good = {2, 3}, below = {1};
  return code == 0 ? none : code == 1 ? good : below;
}

static int pipeline(int most) {
  std::vector<std::unique_ptr<GpuBackend>> pool;
  pool.emplace_back(new GpuBackend());
  std::vector<std::vector<int>> axes = {{0, 1}, {0, 1, 2}, {0, 3}, {0, 1, 2}, {-2, 4, 200}, {0, 1}, {0, 3, -5}, {0, 1, 2}, {-2, 0x5B, 300}, {0, 1},
                                        {0, 1, 2}, {0, 1, 2}, {0, 3, -7}, {-1, 2, 70000}, {0, 1}, {0}};
  std::vector<std::vector<int>> cases;
  combos(axes, most, cases);
  // the fields that say "take the options", under every single option and every pair of them
  for (int bits = 0; bits < 128; ++bits)
    if (__builtin_popcount((unsigned)bits) <= 2)
      for (int kc : {0, 1}) cases.push_back({kc, 0, -1, 0, -1, 0, -1, 0, -1, 0, 0, 0, -1, -1, 0, bits});
  for (const std::vector<int> &c : cases) {
    const int o = c[15];
    blob_options().min_blob_cells = o & 1 ? 3 : 0;
    gmc_options().max_shift = o & 2 ? 4 : -1; gmc_options().vectors = (o & 2) != 0;
    gmc_blob_options().min_blob_cells = o & 4 ? 3 : 0;
    dir_options().allow = o & 8 ? 0x5B : -1; dir_options().sectors = (o & 8) != 0;
    plane_options().plane = plane_of(o & 16 ? 1 : 0);
    persist_options().min_run = o & 32 ? 3 : 0; persist_options().reach = o & 32 ? 2 : -1;
    centre_options().keep = (o & 64) != 0;
    PipelineResult r;
    r.keep_centres = c[0] != 0; r.sweep_levels = levels(c[1]);
    r.min_blob_cells = c[2]; r.blob_sweep_levels = levels(c[3]);
    r.gmc_max_shift = c[4]; r.gmc_vectors = c[5] != 0;
    r.gmc_blob_cells = c[6]; r.gmc_blob_sweep_levels = levels(c[7]);
    r.dir_allow = c[8]; r.dir_sectors = c[9] != 0;
    r.dir_plane = plane_of(c[10]);
    r.keep = keep_of(c[11]);
    r.min_run = c[12]; r.reach = c[13]; r.run_sweep_levels = c[14] ? std::vector<int>{2, 4} : std::vector<int>();
    const int rc = run_scan_pipeline([] { return std::unique_ptr<FrameSource>(new Clip()); }, 1, r, 0, &pool);
    std::printf("P %s\t%d\t%llu\t%s\n", join(c).c_str(), rc, (unsigned long long)r.frames_scanned, r.error.empty() ? "-" : r.error.c_str());
  }
  return 0;
}

// The six things a video can ask, as scanner cases; under a keep mask where `masked`.
static std::vector<int> asks(int mode, bool masked) {
  std::vector<int> c = {1, 0, 0, -1, 0, 0, MT_PIPE_REPORT_CENTRES, -1, 0, 0, masked ? 1 : 0, -1};
  if (mode == 1) { c[1] = 3; c[2] = 1; }
  if (mode == 2) { c[3] = 4; c[4] = 1; }
  if (mode == 3) { c[5] = 3; c[6] = MT_PIPE_REPORT_LARGEST; }
  if (mode == 4) { c[7] = 0x5B; c[8] = 1; }
  if (mode == 5) { c[9] = 1; c[8] = 1; }
  return c;
}

static int pooled() {
  Clip clip;
  GpuBackend be;
  for (int x = 0; x < 6; ++x)
    for (int y = 0; y < 6; ++y) {
      std::string err;
      if (!init_scanner(clip, be, asks(x, (x + y) % 2 == 0), err)) { std::printf("Q %d %d\tprevious video: %s\t-\n", x, y, err.c_str()); continue; }
      const bool ok = init_scanner(clip, be, asks(y, y % 2 == 1), err);
      std::printf("Q %d %d\t%s\t%s\n", x, y, ok ? "ok" : err.c_str(), state(be.pipe()).c_str());
    }
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s scanner [full | N] | pipeline N | pooled\n", argv[0]); return 2; }
  try {
    Config::load_all();
    mt_scan_params p;
    if (mtgpu_params_from_config(&p, Clip::kW, Clip::kH, Config::mv_threshold_sq(), Config::block_size(), Config::block_shift(),
                                 Config::vectors_needed(), Config::clusters_needed(), Config::vertical_mask()) != MT_OK) {
      std::fprintf(stderr, "error: %s\n", mtgpu_last_error());
      return 1;
    }
    g_gw = p.grid_w; g_gh = p.grid_h;
    std::printf("grid %d %d\n", g_gw, g_gh);
    const int most = argc > 2 && std::strcmp(argv[2], "full") != 0 ? std::atoi(argv[2]) : -1;
    if (!std::strcmp(argv[1], "scanner")) return scanner(most);
    if (!std::strcmp(argv[1], "pipeline")) return pipeline(most);
    if (!std::strcmp(argv[1], "pooled")) return pooled();
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "unknown subcommand %s\n", argv[1]);
  return 2;
}
