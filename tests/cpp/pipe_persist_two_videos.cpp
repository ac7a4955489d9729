// pipe_persist_two_videos.cpp — one worker pool, three videos, a persistence setting and a boxed pipe that must not leak
// (tests/test_gpu_pipe_persist.py):
//   pipe_persist_two_videos STREAM.mtmv THREADS
// runs run_scan_pipeline (csrc/host/mtgpu_host.hpp) three times on the SAME pool of GpuBackends, as process_batch does
// for the videos of one stream: the recording under min_blob_cells 1 with persistence and boxes (min_run 3, reach 1), the
// recording with nothing (min_run 0: off whatever persist_options() says), and the recording under persistence without
// boxes (min_run 3, no blob mode).  After each run it prints
//   run <i> rc <rc> layouts <l0,l1,...> motion_frames <n> before <n> frames_scanned <n> traced <n> boxed <n> runs <n> timestamps <t0,t1,...>
// (layouts: mtgpu_pipe_stats.layout of every backend of the pool that holds a pipe; traced: entries of the pooled trace;
// boxed: those whose box is not the all-0xFFFF one; runs: entries of `runs`; timestamps sorted, %.17g).
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
    for (int run = 0; run < 3; ++run) {
      PipelineResult r;
      r.min_blob_cells = run == 0 ? 1 : 0;
      r.min_run = run == 1 ? 0 : 3;
      r.reach = run == 0 ? 1 : -1;
      const int rc = run_scan_pipeline([&]() -> std::unique_ptr<FrameSource> { return std::unique_ptr<FrameSource>(new MtmvSource(file)); },
                                       threads, r, 0, &pool);
      if (rc != 0) { std::fprintf(stderr, "error: run %d: %s\n", run, r.error.c_str()); return 1; }
      std::printf("run %d rc %d layouts ", run, rc);
      bool first = true;
      for (auto &b : pool)
        if (b->pipe()) {
          mtgpu_pipe_stats st;
          if (mtgpu_pipe_get_stats(b->pipe(), &st) != MT_OK) { std::fprintf(stderr, "error: %s\n", mtgpu_last_error()); return 1; }
          std::printf("%s%d", first ? "" : ",", (int)st.layout);
          first = false;
        }
      size_t boxed = 0;
      for (const TraceEntry &e : r.trace) boxed += (e.box.x0 & e.box.y0 & e.box.x1 & e.box.y1) != 0xffffu;
      std::vector<double> ts = r.timestamps;
      std::sort(ts.begin(), ts.end());
      std::printf(" motion_frames %zu before %zu frames_scanned %llu traced %zu boxed %zu runs %zu timestamps ", r.motion_frames,
                  r.frames_before_persist, (unsigned long long)r.frames_scanned, r.trace.size(), boxed, r.runs.size());
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
