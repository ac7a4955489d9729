// scan_request_replay.cpp — csrc/host/scan_request.hpp alone (no HIP, no library; tests/test_scan_request_host.py builds it
// with the address and undefined-behaviour sanitizers): the cases of tests/cpp/mode_matrix_probe.cpp, read from stdin in
// the probe's encodings, through the two pure functions.
//   scan_request_replay GW GH
//   in:  S <12 numbers> | P <16 numbers>
//   out: S <case>\t<ok | error text>\t<the pipe state the request stands for, "-" with an error>
//        P <case>\t<error text or ->\t<gmc_on pair_on pair_largest report_largest dir_on plane_on persist_on keep_centres>
// A pipeline case that resolve_pipeline accepts goes on to resolve_scanner with the values run_scan_pipeline hands its
// scanners (its scanners[i]->set_* lines), and that answer is printed.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "scan_request.hpp"

using namespace mtgpu_host;

static int g_gw = 0, g_gh = 0;
static size_t plane_bytes(int code) { return code ? (size_t)g_gw * g_gh - (code == 2) : 0; }
static size_t keep_words(int code) { return code ? (size_t)g_gh * ((g_gw + 63) / 64) + (code == 2) : 0; }

static std::string state(const ScanRequest &r, bool keep) {
  char t[256];
  const bool b = r.mode == ScanMode::blobs, g = r.mode == ScanMode::gmc, p = r.mode == ScanMode::gmc_blobs, d = r.mode == ScanMode::dir,
             l = r.mode == ScanMode::plane;
  std::snprintf(t, sizeof t, "keep=%d blobs=%d:%d:%d gmc=%d:%d:%d:%d pair=%d:%d:%d:%d:%d dir=%d:%d:%d plane=%d:%d", keep ? 1 : 0, b, b ? r.min_blob : 0,
                b ? r.report : 0, g, g ? r.max_shift : 0, g ? r.min_share_q8 : 0, g ? r.report : 0, p, p ? r.min_blob : 0, p ? r.max_shift : 0,
                p ? r.min_share_q8 : 0, p ? r.report : 0, d, d ? r.allow : 0, d ? r.report : 0, l, l ? r.report : 0);
  return t;
}

struct Fields {   // a PipelineResult's input fields
  bool keep_centres = false;
  std::vector<int> sweep_levels;
  int min_blob_cells = -1;
  std::vector<int> blob_sweep_levels;
  int gmc_max_shift = -1, gmc_min_share_q8 = MTGPU_GMC_DEFAULT_MIN_SHARE_Q8;
  bool gmc_vectors = false;
  int gmc_blob_cells = -1, gmc_blob_max_shift = MTGPU_GMC_DEFAULT_MAX_SHIFT, gmc_blob_min_share_q8 = MTGPU_GMC_DEFAULT_MIN_SHARE_Q8;
  std::vector<int> gmc_blob_sweep_levels;
  int dir_allow = -1;
  bool dir_sectors = false;
  std::vector<uint8_t> dir_plane;
  int min_run = -1;
  uint32_t max_dropout = 0;
  int reach = -1;
  std::vector<int> run_sweep_levels;
};

static std::vector<int> levels(int code) { return code == 0 ? std::vector<int>() : code == 1 ? std::vector<int>{2, 3} : std::vector<int>{1}; }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  g_gw = std::atoi(argv[1]); g_gh = std::atoi(argv[2]);
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    std::vector<int> c;
    for (int v; in >> v;) c.push_back(v);
    const std::string text = line.substr(2);
    if (kind == "S" && c.size() == 12) {
      ScannerAsk a;
      a.keep_centres = c[0]; a.min_blob_cells = c[1]; a.report_largest = c[2]; a.gmc_max_shift = c[3]; a.report_vector = c[4];
      a.gmc_blob_cells = c[5]; a.gmc_blob_report = c[6]; a.dir_allow = c[7]; a.report_sectors = c[8];
      a.plane_bytes = plane_bytes(c[9]); a.keep_words = keep_words(c[10]); a.persist_reach = c[11] >= 0 ? c[11] : -1;
      a.grid_w = g_gw; a.grid_h = g_gh;
      const ScanRequest r = resolve_scanner(a);
      std::printf("S %s\t%s\t%s\n", text.c_str(), r.error.empty() ? "ok" : r.error.c_str(), r.error.empty() ? state(r, a.keep_words != 0).c_str() : "-");
    } else if (kind == "P" && c.size() == 16) {
      const int o = c[15];
      CentreOptions co; BlobOptions bo; GmcOptions go; GmcBlobOptions po; DirOptions dio; PlaneOptions plo; PersistOptions pso;
      bo.min_blob_cells = o & 1 ? 3 : 0;
      go.max_shift = o & 2 ? 4 : -1; go.vectors = (o & 2) != 0;
      po.min_blob_cells = o & 4 ? 3 : 0;
      dio.allow = o & 8 ? 0x5B : -1; dio.sectors = (o & 8) != 0;
      plo.plane.assign(plane_bytes(o & 16 ? 1 : 0), 0x5B);
      pso.min_run = o & 32 ? 3 : 0; pso.reach = o & 32 ? 2 : -1;
      co.keep = (o & 64) != 0;
      Fields f;
      f.keep_centres = c[0]; f.sweep_levels = levels(c[1]); f.min_blob_cells = c[2]; f.blob_sweep_levels = levels(c[3]);
      f.gmc_max_shift = c[4]; f.gmc_vectors = c[5]; f.gmc_blob_cells = c[6]; f.gmc_blob_sweep_levels = levels(c[7]);
      f.dir_allow = c[8]; f.dir_sectors = c[9]; f.dir_plane.assign(plane_bytes(c[10]), 0x5B);
      f.min_run = c[12]; f.reach = c[13];
      if (c[14]) f.run_sweep_levels = {2, 4};
      const PipelineModes m = resolve_pipeline(f, PipelineDefaults{co, bo, go, po, dio, plo, pso}, 2);
      std::string err = m.error;
      if (err.empty()) {   // what run_scan_pipeline hands every worker's scanner
        ScannerAsk a;
        a.keep_centres = m.keep_centres;
        a.keep_words = keep_words(c[11]);
        a.min_blob_cells = f.min_blob_cells; a.report_largest = m.report_largest;
        a.gmc_max_shift = m.gmc_on ? f.gmc_max_shift : -1; a.gmc_min_share_q8 = f.gmc_min_share_q8; a.report_vector = f.gmc_vectors;
        a.gmc_blob_cells = m.pair_on ? std::max(1, f.gmc_blob_cells) : 0; a.gmc_blob_max_shift = f.gmc_blob_max_shift;
        a.gmc_blob_min_share_q8 = f.gmc_blob_min_share_q8;
        a.gmc_blob_report = m.pair_largest ? MT_PIPE_REPORT_LARGEST : MT_PIPE_REPORT_CENTRES;
        a.dir_allow = m.dir_on ? f.dir_allow : -1; a.report_sectors = f.dir_sectors;
        a.plane_bytes = f.dir_plane.size();
        a.persist_reach = m.persist_on ? f.reach : -1;
        a.grid_w = g_gw; a.grid_h = g_gh;
        err = resolve_scanner(a).error;
      }
      std::printf("P %s\t%s\t%d %d %d %d %d %d %d %d\n", text.c_str(), err.empty() ? "-" : err.c_str(), m.gmc_on, m.pair_on, m.pair_largest, m.report_largest,
                  m.dir_on, m.plane_on, m.persist_on, m.keep_centres);
    } else {
      return 3;
    }
  }
  return 0;
}
