// pipe_blobs_two_videos.cpp — one worker pool, several videos, a blob setting that must not leak
// (tests/test_gpu_pipe_blobs.py):
//   pipe_blobs_two_videos STREAM.mtmv MIN_BLOB_CELLS THREADS
// runs run_scan_pipeline (csrc/host/mtgpu_host.hpp) three times on the SAME pool of GpuBackends, as process_batch does
// for the videos of one stream: the recording under MIN_BLOB_CELLS, the recording without the rule, the recording under
// MIN_BLOB_CELLS with the largest blobs reported and swept at that level.  After each run it prints
//   run <i> blobs <b0,b1,...> motion_frames <n> frames_scanned <n> sweep_frames <n> timestamps <t0,t1,...>
// (blobs: mtgpu_pipe_blobs' min_blob_cells of every backend of the pool that holds a pipe, 0 where the scan is off, with
// an `L` behind it where the pipe reports the largest blob; sweep_frames: n_timestamps of the one blob_sweep entry, -1
// without one; timestamps sorted, %.17g).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "mtgpu_host.hpp"

using namespace mtgpu_host;

int main(int argc, char **argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: %s STREAM.mtmv MIN_BLOB_CELLS THREADS\n", argv[0]); return 2; }
  const int min_blob = std::atoi(argv[2]);
  const int threads = std::atoi(argv[3]);
  try {
    Config::load_all();
    MtmvFile file(argv[1]);
    std::vector<std::unique_ptr<GpuBackend>> pool;
    for (int i = 0; i < threads; ++i) pool.emplace_back(new GpuBackend());
    for (int run = 0; run < 3; ++run) {
      PipelineResult r;
      r.min_blob_cells = run != 1 ? min_blob : 0;
      if (run == 2) r.blob_sweep_levels = {min_blob};
      const int rc = run_scan_pipeline([&]() -> std::unique_ptr<FrameSource> { return std::unique_ptr<FrameSource>(new MtmvSource(file)); },
                                       threads, r, 0, &pool);
      if (rc != 0) { std::fprintf(stderr, "error: run %d: %s\n", run, r.error.c_str()); return 1; }
      std::printf("run %d blobs ", run);
      bool first = true;
      for (auto &b : pool)
        if (b->pipe()) {
          int32_t n = 0;
          int report = 0;
          const int on = mtgpu_pipe_blobs(b->pipe(), &n, &report);
          std::printf("%s%d%s", first ? "" : ",", on == 1 ? (int)n : on, on == 1 && report == MT_PIPE_REPORT_LARGEST ? "L" : "");
          first = false;
        }
      std::vector<double> ts = r.timestamps;
      std::sort(ts.begin(), ts.end());
      std::printf(" motion_frames %zu frames_scanned %llu sweep_frames %lld timestamps ", r.motion_frames,
                  (unsigned long long)r.frames_scanned, r.blob_sweep.empty() ? -1ll : (long long)r.blob_sweep[0].merge.n_timestamps);
      for (size_t i = 0; i < ts.size(); ++i) std::printf("%s%.17g", i ? "," : "", ts[i]);
      std::printf("\n");
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
