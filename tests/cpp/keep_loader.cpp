// keep_loader.cpp — mtgpu_host::load_keep (csrc/host/mtgpu_host.hpp) from the outside, for tests/test_pipe_zones_host.py:
//   keep_loader FILE.mtkeep GRID_W GRID_H
// prints "ok" and the gh * W keep words in hexadecimal, one row per line — or "error <message>" (exit status 3).
// Stand-alone on purpose: the parser touches nothing of the device, so this program can also be built with
// -fsanitize=address,undefined and run on any machine.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mtgpu_host.hpp"

int main(int argc, char **argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: %s FILE.mtkeep GRID_W GRID_H\n", argv[0]); return 2; }
  const int gw = std::atoi(argv[2]), gh = std::atoi(argv[3]);
  std::vector<uint64_t> words;
  std::string err;
  if (!mtgpu_host::load_keep(argv[1], gw, gh, words, err)) {
    std::printf("error %s\nwords %zu\n", err.c_str(), words.size());
    return 3;
  }
  const size_t W = ((size_t)gw + 63u) / 64u;
  std::printf("ok\n");
  for (int y = 0; y < gh; ++y) {
    for (size_t w = 0; w < W; ++w) std::printf("%s%016llx", w ? " " : "", (unsigned long long)words[(size_t)y * W + w]);
    std::printf("\n");
  }
  return 0;
}
