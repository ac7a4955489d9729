// pipe_lanes_two_videos.cpp — one worker pool, several videos, a direction plane that must not leak
// (tests/test_gpu_pipe_lanes.py):
//   pipe_lanes_two_videos STREAM.mtmv THREADS PLANE.mtdir GW GH
// runs run_scan_pipeline (csrc/host/mtgpu_host.hpp) five times on the SAME pool of GpuBackends, as process_batch does for
// the videos of one stream: the recording under the plane, the recording without it, the recording under the plane with
// the sector words reported, and — two conflicts that must be refused before any decode — the plane together with
// dir_allow 0xFF and the plane together with min_blob_cells 3.  After each run it prints
//   run <i> rc <rc> plane <d0,d1,...> motion_frames <n> frames_scanned <n> frames <n> present <p0:..:p7> dominant <d0:..:d7> timestamps <t0,t1,...>
// (plane: mtgpu_pipe_plane's answer for every backend of the pool that holds a pipe — 1 where the plane is on and equals
// the file's bytes, 0 where it is off, 9 where it is on with other bytes — with an `S` behind it where the pipe reports the
// sector word, and mtgpu_pipe_dir's answer behind a `/`; timestamps sorted, %.17g).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "mtgpu_host.hpp"

using namespace mtgpu_host;

int main(int argc, char **argv) {
  if (argc != 6) { std::fprintf(stderr, "usage: %s STREAM.mtmv THREADS PLANE.mtdir GW GH\n", argv[0]); return 2; }
  const int threads = std::atoi(argv[2]);
  try {
    Config::load_all();
    MtmvFile file(argv[1]);
    std::vector<uint8_t> plane;
    std::string err;
    if (!load_plane(argv[3], std::atoi(argv[4]), std::atoi(argv[5]), plane, err)) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 1; }
    std::vector<std::unique_ptr<GpuBackend>> pool;
    for (int i = 0; i < threads; ++i) pool.emplace_back(new GpuBackend());
    for (int run = 0; run < 5; ++run) {
      PipelineResult r;
      r.dir_allow = run == 3 ? 0xFF : -2;
      if (run != 1) r.dir_plane = plane;
      r.dir_sectors = run == 2;
      r.min_blob_cells = run == 4 ? 3 : 0;
      const int rc = run_scan_pipeline([&]() -> std::unique_ptr<FrameSource> { return std::unique_ptr<FrameSource>(new MtmvSource(file)); },
                                       threads, r, 0, &pool);
      if (rc != 0 && run < 3) { std::fprintf(stderr, "error: run %d: %s\n", run, r.error.c_str()); return 1; }
      if (run >= 3) {
        std::printf("run %d rc %d frames_scanned %llu error %s\n", run, rc, (unsigned long long)r.frames_scanned, r.error.c_str());
        continue;
      }
      std::printf("run %d rc %d plane ", run, rc);
      bool first = true;
      for (auto &b : pool)
        if (b->pipe()) {
          std::vector<uint8_t> back(plane.size(), 0);
          int report = 0;
          const int on = mtgpu_pipe_plane(b->pipe(), back.data(), &report);
          std::printf("%s%d%s/%d", first ? "" : ",", on == 1 ? (back == plane ? 1 : 9) : on, on == 1 && report == MT_PIPE_REPORT_SECTORS ? "S" : "",
                      mtgpu_pipe_dir(b->pipe(), nullptr, nullptr));
          first = false;
        }
      std::vector<double> ts = r.timestamps;
      std::sort(ts.begin(), ts.end());
      std::printf(" motion_frames %zu frames_scanned %llu frames %llu present ", r.motion_frames, (unsigned long long)r.frames_scanned,
                  (unsigned long long)r.dir_frames);
      for (int k = 0; k < 8; ++k) std::printf("%s%llu", k ? ":" : "", (unsigned long long)r.dir_present_frames[k]);
      std::printf(" dominant ");
      for (int k = 0; k < 8; ++k) std::printf("%s%llu", k ? ":" : "", (unsigned long long)r.dir_dominant_frames[k]);
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
