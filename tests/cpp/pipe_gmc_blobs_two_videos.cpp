// pipe_gmc_blobs_two_videos.cpp — one worker pool, several videos, a pair setting that must not leak
// (tests/test_gpu_pipe_gmc_blobs.py):
//   pipe_gmc_blobs_two_videos STREAM.mtmv THREADS
// runs run_scan_pipeline (csrc/host/mtgpu_host.hpp) four times on the SAME pool of GpuBackends, as process_batch does
// for the videos of one stream: the recording under the compensated blob scan at 5 cells and the defaults, the recording
// plainly, the recording under the pair at 31 cells and max_shift 3, and — a conflict that must be refused before any
// decode — the pair together with min_blob_cells 3.  After each run it prints
//   run <i> rc <rc> pair <p0,p1,...> motion_frames <n> frames_scanned <n> timestamps <t0,t1,...>
// (pair: mtgpu_pipe_gmc_blobs's min_blob_cells:max_shift of every backend of the pool that holds a pipe, - where the pair
// is off; timestamps sorted, %.17g).
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
      r.gmc_blob_cells = run == 0 ? 5 : run == 1 ? 0 : run == 2 ? 31 : 3;
      if (run == 2) r.gmc_blob_max_shift = 3;
      r.min_blob_cells = run == 3 ? 3 : 0;
      const int rc = run_scan_pipeline([&]() -> std::unique_ptr<FrameSource> { return std::unique_ptr<FrameSource>(new MtmvSource(file)); },
                                       threads, r, 0, &pool);
      if (rc != 0 && run != 3) { std::fprintf(stderr, "error: run %d: %s\n", run, r.error.c_str()); return 1; }
      if (run == 3) {
        std::printf("run 3 rc %d frames_scanned %llu error %s\n", rc, (unsigned long long)r.frames_scanned, r.error.c_str());
        continue;
      }
      std::printf("run %d rc %d pair ", run, rc);
      bool first = true;
      for (auto &b : pool)
        if (b->pipe()) {
          int32_t cells = 0, ms = 0;
          const int on = mtgpu_pipe_gmc_blobs(b->pipe(), &cells, &ms, nullptr, nullptr);
          if (on == 1) std::printf("%s%d:%d", first ? "" : ",", (int)cells, (int)ms);
          else std::printf("%s-", first ? "" : ",");
          first = false;
        }
      std::vector<double> ts = r.timestamps;
      std::sort(ts.begin(), ts.end());
      std::printf(" motion_frames %zu frames_scanned %llu timestamps ", r.motion_frames, (unsigned long long)r.frames_scanned);
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
