// pipe_zones_two_videos.cpp — one worker pool, several videos, masks that must not leak (tests/test_gpu_pipe_zones.py):
//   pipe_zones_two_videos STREAM.mtmv MASK.mtkeep THREADS
// runs run_scan_pipeline (csrc/host/mtgpu_host.hpp) three times on the SAME pool of GpuBackends, as process_batch does
// for the videos of one stream: the recording under the mask, the recording without one, the recording under the mask
// again.  After each run it prints
//   run <i> keep <words> has_keep <h0,h1,...> motion_frames <n> frames_scanned <n> timestamps <t0,t1,...>
// (has_keep: mtgpu_pipe_has_keep of every backend of the pool that holds a pipe; timestamps sorted, %.17g).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "mtgpu_host.hpp"

using namespace mtgpu_host;

int main(int argc, char **argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: %s STREAM.mtmv MASK.mtkeep THREADS\n", argv[0]); return 2; }
  const int threads = std::atoi(argv[3]);
  try {
    Config::load_all();
    MtmvFile file(argv[1]);
    mt_scan_params p;
    if (mtgpu_params_from_config(&p, (int)file.hdr->width, (int)file.hdr->height, Config::mv_threshold_sq(), Config::block_size(),
                                 Config::block_shift(), Config::vectors_needed(), Config::clusters_needed(),
                                 Config::vertical_mask()) != MT_OK) {
      std::fprintf(stderr, "error: %s\n", mtgpu_last_error());
      return 1;
    }
    std::vector<uint64_t> mask;
    std::string err;
    if (!load_keep(argv[2], p.grid_w, p.grid_h, mask, err)) { std::fprintf(stderr, "error: %s\n", err.c_str()); return 1; }
    std::vector<std::unique_ptr<GpuBackend>> pool;
    for (int i = 0; i < threads; ++i) pool.emplace_back(new GpuBackend());
    for (int run = 0; run < 3; ++run) {
      PipelineResult r;
      if (run != 1) r.keep = mask;
      const int rc = run_scan_pipeline([&]() -> std::unique_ptr<FrameSource> { return std::unique_ptr<FrameSource>(new MtmvSource(file)); },
                                       threads, r, 0, &pool);
      if (rc != 0) { std::fprintf(stderr, "error: run %d: %s\n", run, r.error.c_str()); return 1; }
      std::printf("run %d keep %zu has_keep ", run, r.keep.size());
      bool first = true;
      for (auto &b : pool)
        if (b->pipe()) { std::printf("%s%d", first ? "" : ",", mtgpu_pipe_has_keep(b->pipe())); first = false; }
      std::vector<double> ts = r.timestamps;
      std::sort(ts.begin(), ts.end());
      std::printf(" motion_frames %zu frames_scanned %llu timestamps ", r.motion_frames, (unsigned long long)r.frames_scanned);
      for (size_t i = 0; i < ts.size(); ++i) std::printf("%s%.17g", i ? "," : "", ts[i]);
      std::printf("\n");
    }
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
