// pipe_gmc_two_videos.cpp — one worker pool, several videos, a compensation setting that must not leak
// (tests/test_gpu_pipe_gmc.py):
//   pipe_gmc_two_videos STREAM.mtmv THREADS
// runs run_scan_pipeline (csrc/host/mtgpu_host.hpp) four times on the SAME pool of GpuBackends, as process_batch does
// for the videos of one stream: the recording compensated at the defaults, the recording without compensation, the
// recording compensated at max_shift 3 with the applied vectors reported, and — a conflict that must be refused before
// any decode — compensation together with min_blob_cells 3.  After each run it prints
//   run <i> rc <rc> gmc <g0,g1,...> motion_frames <n> frames_scanned <n> moved <n> top <gx:gy:frames,...> timestamps <t0,t1,...>
// (gmc: mtgpu_pipe_gmc's max_shift of every backend of the pool that holds a pipe, -1 where compensation is off, with a
// `V` behind it where the pipe reports the vector; timestamps sorted, %.17g).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "mtgpu_host.hpp"

using namespace mtgpu_host;

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s STREAM.mtmv THREADS\n", argv[0]); return 2; }
  const int threads = std::atoi(argv[2]);
  try {
    Config::load_all();
    MtmvFile file(argv[1]);
    std::vector<std::unique_ptr<GpuBackend>> pool;
    for (int i = 0; i < threads; ++i) pool.emplace_back(new GpuBackend());
    for (int run = 0; run < 4; ++run) {
      PipelineResult r;
      r.gmc_max_shift = run == 0 ? MTGPU_GMC_DEFAULT_MAX_SHIFT : run == 1 ? -2 : 3;
      r.gmc_vectors = run == 2;
      r.min_blob_cells = run == 3 ? 3 : 0;
      const int rc = run_scan_pipeline([&]() -> std::unique_ptr<FrameSource> { return std::unique_ptr<FrameSource>(new MtmvSource(file)); },
                                       threads, r, 0, &pool);
      if (rc != 0 && run != 3) { std::fprintf(stderr, "error: run %d: %s\n", run, r.error.c_str()); return 1; }
      if (run == 3) {
        std::printf("run 3 rc %d frames_scanned %llu error %s\n", rc, (unsigned long long)r.frames_scanned, r.error.c_str());
        continue;
      }
      std::printf("run %d rc %d gmc ", run, rc);
      bool first = true;
      for (auto &b : pool)
        if (b->pipe()) {
          int32_t ms = 0;
          int report = 0;
          const int on = mtgpu_pipe_gmc(b->pipe(), &ms, nullptr, &report);
          std::printf("%s%d%s", first ? "" : ",", on == 1 ? (int)ms : -1, on == 1 && report == MT_PIPE_REPORT_VECTOR ? "V" : "");
          first = false;
        }
      std::vector<double> ts = r.timestamps;
      std::sort(ts.begin(), ts.end());
      std::printf(" motion_frames %zu frames_scanned %llu moved %llu top ", r.motion_frames, (unsigned long long)r.frames_scanned,
                  (unsigned long long)r.gmc_moved_frames);
      for (size_t i = 0; i < r.gmc_top.size(); ++i)
        std::printf("%s%d:%d:%llu", i ? "," : "", r.gmc_top[i].gx, r.gmc_top[i].gy, (unsigned long long)r.gmc_top[i].frames);
      if (r.gmc_top.empty()) std::printf("-");
      std::printf(" timestamps ");
      for (size_t i = 0; i < ts.size(); ++i) std::printf("%s%.17g", i ? "," : "", ts[i]);
      if (ts.empty()) std::printf("-");
      std::printf("\n");
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
