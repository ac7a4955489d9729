// scan_request.hpp — what a video asks of its pipe, settled once.  No HIP, no library call: two pure functions over plain
// values, included by mtgpu_host.hpp and, alone, by a sanitized program of the CPU tests (tests/test_scan_request_host.py).
//   resolve_scanner    what a GpuMotionScanner was told through its setters -> the ONE mode its pipe runs, with its
//                      settings and report code, or the sentence that refuses the combination
//   resolve_pipeline   a PipelineResult's input fields and the process-wide options -> the defaults filled in and the
//                      derived booleans run_scan_pipeline works with, or the sentence
// A pipe runs one of six scans (include/mtgpu_pipe_*.h) and the modes exclude each other, so both functions hold their
// "not together" rules as a table: one row per (mode asked for, what else was asked for).  Rows are read in order, and a
// mode's rows stand where the rule stood when each mode had a block of its own: the FIRST broken rule is the answer.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#include "mtgpu.h"

namespace mtgpu_host {

enum class ScanMode { plain, blobs, gmc, gmc_blobs, dir, plane };

// One row of a pairwise table: `mode` is asked for together with any of the things in `with` (bits of the function's own).
struct NotTogether { ScanMode mode; unsigned with; const char *text; };

template <size_t N>
inline const char *not_together(const NotTogether (&rows)[N], ScanMode mode, unsigned asked) {
  for (const NotTogether &r : rows)
    if (r.mode == mode && (r.with & asked)) return r.text;
  return nullptr;
}

// ---------------------------------------------------------------- a scanner's setters -> its pipe's one mode

struct ScannerAsk {            // GpuMotionScanner's setters, as values
  bool keep_centres = false, report_largest = false, report_vector = false, report_sectors = false;
  int min_blob_cells = 0;      // set_min_blob_cells; 0: off
  int gmc_max_shift = -1, gmc_min_share_q8 = MTGPU_GMC_DEFAULT_MIN_SHARE_Q8;   // set_gmc; max_shift < 0: off
  int gmc_blob_cells = 0;      // set_gmc_blobs; 0: off
  int gmc_blob_max_shift = MTGPU_GMC_DEFAULT_MAX_SHIFT, gmc_blob_min_share_q8 = MTGPU_GMC_DEFAULT_MIN_SHARE_Q8;
  int gmc_blob_report = MT_PIPE_REPORT_CENTRES;   // report_gmc_blobs
  int dir_allow = -1;          // set_dir; -1: off
  size_t plane_bytes = 0;      // set_plane's size; 0: none
  size_t keep_words = 0;       // set_keep's size; 0: none
  int grid_w = 0, grid_h = 0;  // the context's grid
  int persist_reach = -1;      // set_persist
};

struct ScanRequest {
  std::string error;           // empty: the rest holds
  ScanMode mode = ScanMode::plain;
  int min_blob = 0, max_shift = 0, min_share_q8 = 0, allow = 0, report = MT_PIPE_REPORT_CENTRES;   // what the mode's setter takes
};

// The two rungs that need no grid: GpuMotionScanner::initialize asks them before it builds a pipe.
inline std::string persist_error(const ScannerAsk &a) {
  if (a.persist_reach >= 0 && a.min_blob_cells <= 0 && a.gmc_blob_cells <= 0)
    return "set_persist with reach >= 0 needs set_min_blob_cells(n > 0) or set_gmc_blobs(n > 0): only a blob scan reports the box "
           "that reach compares";
  if (a.persist_reach > 65535) return "set_persist: reach " + std::to_string(a.persist_reach) + " outside [0,65535]";
  return std::string();
}

enum : unsigned { S_MIN_BLOB = 1, S_LARGEST = 2, S_GMC = 4, S_VECTOR = 8, S_PAIR = 16, S_DIR = 32 };
static const NotTogether SCANNER_NOT_TOGETHER[] = {
    {ScanMode::gmc, S_MIN_BLOB | S_LARGEST, "compensation and blobs are not together yet"},
    {ScanMode::gmc_blobs, S_MIN_BLOB, "set_gmc_blobs together with set_min_blob_cells: the compensated blob scan has its own minimum blob size"},
    {ScanMode::gmc_blobs, S_LARGEST, "set_gmc_blobs together with report_largest: ask report_gmc_blobs(MT_PIPE_REPORT_LARGEST)"},
    {ScanMode::gmc_blobs, S_GMC, "set_gmc_blobs together with set_gmc: the compensated blob scan has its own max_shift and min_share_q8"},
    {ScanMode::gmc_blobs, S_VECTOR, "set_gmc_blobs together with report_vector: ask report_gmc_blobs(MT_PIPE_REPORT_VECTOR)"},
    {ScanMode::dir, S_MIN_BLOB | S_LARGEST, "set_dir together with set_min_blob_cells / report_largest: direction and blobs are not together yet"},
    {ScanMode::dir, S_GMC | S_VECTOR, "set_dir together with set_gmc / report_vector: direction and compensation are not together yet"},
    {ScanMode::dir, S_PAIR, "set_dir together with set_gmc_blobs: direction and the compensated blob scan are not together yet"},
    {ScanMode::plane, S_DIR, "set_plane together with set_dir: a plane and the allow byte are one rule at two granularities"},
    {ScanMode::plane, S_MIN_BLOB | S_LARGEST, "set_plane together with set_min_blob_cells / report_largest: planes and blobs are not together yet"},
    {ScanMode::plane, S_GMC | S_VECTOR, "set_plane together with set_gmc / report_vector: planes and compensation are not together yet"},
    {ScanMode::plane, S_PAIR, "set_plane together with set_gmc_blobs: planes and the compensated blob scan are not together yet"}};

// Check order: persist, blobs, gmc, keep size, pair, dir, plane.  Every later mode's rows refuse every earlier one, so at
// most one mode is left standing at the end.
inline ScanRequest resolve_scanner(const ScannerAsk &a) {
  ScanRequest r;
  auto refuse = [&r](std::string text) { r.error = std::move(text); return r; };
  auto grid = [&a](size_t have, const char *unit, size_t want) {
    return std::to_string(have) + unit + std::to_string(a.grid_w) + "x" + std::to_string(a.grid_h) + " grid takes " + std::to_string(want);
  };
  const unsigned asked = (a.min_blob_cells > 0 ? S_MIN_BLOB : 0u) | (a.report_largest ? S_LARGEST : 0u) | (a.gmc_max_shift >= 0 ? S_GMC : 0u) |
                         (a.report_vector ? S_VECTOR : 0u) |
                         (a.gmc_blob_cells != 0 || a.gmc_blob_report != MT_PIPE_REPORT_CENTRES ? S_PAIR : 0u) | (a.dir_allow != -1 ? S_DIR : 0u);
  const char *const sectors_need_centres = "report_sectors needs keep_centres: the sector word travels in the pipe's count array";
  if (!(r.error = persist_error(a)).empty()) return r;
  // blobs
  if (a.min_blob_cells < 0) return refuse("min_blob_cells is " + std::to_string(a.min_blob_cells));
  if (a.report_largest && !a.keep_centres) return refuse("report_largest needs keep_centres: the largest blob travels in the pipe's count array");
  if (asked & (S_MIN_BLOB | S_LARGEST)) {
    r.mode = ScanMode::blobs;
    r.min_blob = a.report_largest ? std::max(1, a.min_blob_cells) : a.min_blob_cells;
    r.report = a.report_largest ? MT_PIPE_REPORT_LARGEST : MT_PIPE_REPORT_CENTRES;
  }
  // compensation
  if (asked & (S_GMC | S_VECTOR)) {
    if (a.gmc_max_shift < 0) return refuse("report_vector needs set_gmc: there is no applied vector without compensation");
    if (const char *t = not_together(SCANNER_NOT_TOGETHER, ScanMode::gmc, asked)) return refuse(t);
    if (a.report_vector && !a.keep_centres) return refuse("report_vector needs keep_centres: the applied vector travels in the pipe's count array");
    r.mode = ScanMode::gmc;
    r.max_shift = a.gmc_max_shift;
    r.min_share_q8 = a.gmc_min_share_q8;
    r.report = a.report_vector ? MT_PIPE_REPORT_VECTOR : MT_PIPE_REPORT_CENTRES;
  }
  // the keep mask's size
  const size_t keep_want = (size_t)a.grid_h * (((size_t)a.grid_w + 63u) / 64u);
  if (a.keep_words != 0 && a.keep_words != keep_want) return refuse("keep mask: " + grid(a.keep_words, " words, the ", keep_want));
  // the compensated blob scan
  if (asked & S_PAIR) {
    if (a.gmc_blob_cells < 0) return refuse("set_gmc_blobs: min_blob_cells is negative");
    if (const char *t = not_together(SCANNER_NOT_TOGETHER, ScanMode::gmc_blobs, asked)) return refuse(t);
    if (a.gmc_blob_report != MT_PIPE_REPORT_CENTRES && !a.keep_centres)
      return refuse("report_gmc_blobs needs keep_centres: the largest blob and the applied vector travel in the pipe's count array");
    r.mode = ScanMode::gmc_blobs;
    r.min_blob = std::max(1, a.gmc_blob_cells);
    r.max_shift = a.gmc_blob_max_shift;
    r.min_share_q8 = a.gmc_blob_min_share_q8;
    r.report = a.gmc_blob_report;
  }
  // the direction byte
  if ((asked & S_DIR) || (a.report_sectors && a.plane_bytes == 0)) {
    if (a.dir_allow == -1) return refuse("report_sectors needs set_dir: there is no sector word without the direction mode");
    if (a.dir_allow < 0 || a.dir_allow > 255) return refuse("set_dir: allow is outside [0,255]");
    if (const char *t = not_together(SCANNER_NOT_TOGETHER, ScanMode::dir, asked)) return refuse(t);
    if (a.report_sectors && !a.keep_centres) return refuse(sectors_need_centres);
    r.mode = ScanMode::dir;
    r.allow = a.dir_allow;
    r.report = a.report_sectors ? MT_PIPE_REPORT_SECTORS : MT_PIPE_REPORT_CENTRES;
  }
  // the direction plane
  if (a.plane_bytes != 0) {
    if (const char *t = not_together(SCANNER_NOT_TOGETHER, ScanMode::plane, asked)) return refuse(t);
    if (a.report_sectors && !a.keep_centres) return refuse(sectors_need_centres);
    const size_t want = (size_t)a.grid_h * (size_t)a.grid_w;
    if (a.plane_bytes != want) return refuse("direction plane: " + grid(a.plane_bytes, " bytes, the ", want));
    r.mode = ScanMode::plane;
    r.report = a.report_sectors ? MT_PIPE_REPORT_SECTORS : MT_PIPE_REPORT_CENTRES;
  }
  return r;
}

// ---------------------------------------------------------------- a pipeline's fields and the options -> what it runs

// Process-wide defaults for a PipelineResult's fields of the same names, as a front end's options set them.
struct PersistOptions {        // --min-run, --max-dropout, --reach, --sweep-min-run; min_run <= 1 and no level: off
  int min_run = 0;
  uint32_t max_dropout = 0;
  int reach = -1;
  std::vector<int> sweep_levels;
};
struct GmcBlobOptions {        // --gmc-blobs, --gmc-blobs-max-shift, --gmc-blobs-min-share-q8, --sweep-gmc-blobs; 0 and no level: off
  int min_blob_cells = 0;
  int max_shift = MTGPU_GMC_DEFAULT_MAX_SHIFT, min_share_q8 = MTGPU_GMC_DEFAULT_MIN_SHARE_Q8;
  std::vector<int> sweep_levels;
};
struct BlobOptions { int min_blob_cells = 0; std::vector<int> sweep_levels; };   // --min-blob-cells, --sweep-blobs
// --gmc, --gmc-max-shift, --gmc-min-share-q8, --gmc-vectors; max_shift < 0: off
struct GmcOptions { int max_shift = -1; int min_share_q8 = MTGPU_GMC_DEFAULT_MIN_SHARE_Q8; bool vectors = false; };
struct DirOptions { int allow = -1; bool sectors = false; };                      // --allow / --ignore, --dir-sectors; allow < 0: off
// ONE plane for every input, read where a pipeline's dir_plane is empty; empty: none.  A front end whose inputs have grids
// of their own hands process_batch a plane_for hook instead.
struct PlaneOptions { std::vector<uint8_t> plane; };
struct CentreOptions { bool keep = false; std::vector<int> sweep_levels; };      // --centres, --sweep

struct PipelineDefaults {      // the seven *_options() singletons of mtgpu_host.hpp, or a test's own
  const CentreOptions &centre; const BlobOptions &blob; const GmcOptions &gmc; const GmcBlobOptions &pair;
  const DirOptions &dir; const PlaneOptions &plane; const PersistOptions &persist;
};

struct PipelineModes {
  std::string error;           // empty: the rest holds
  bool gmc_on = false, pair_on = false, pair_largest = false, report_largest = false, dir_on = false, plane_on = false, persist_on = false, keep_centres = false;
};

enum : unsigned { P_BLOBS = 1, P_GMC = 2, P_PAIR = 4, P_DIR = 8 };
static const NotTogether PIPELINE_NOT_TOGETHER[] = {
    {ScanMode::gmc, P_BLOBS, "compensation together with min_blob_cells / blob_sweep_levels: not together yet"},
    {ScanMode::gmc_blobs, P_BLOBS, "gmc_blob_cells / gmc_blob_sweep_levels together with min_blob_cells / blob_sweep_levels: the compensated blob "
                                   "scan has its own minimum blob size"},
    {ScanMode::gmc_blobs, P_GMC, "gmc_blob_cells / gmc_blob_sweep_levels together with gmc_max_shift / gmc_vectors: the compensated blob scan "
                                 "has its own compensation"},
    {ScanMode::plane, P_DIR, "dir_plane together with dir_allow: a plane and the allow byte are one rule at two granularities"},
    {ScanMode::plane, P_BLOBS, "dir_plane together with min_blob_cells / blob_sweep_levels: planes and blobs are not together yet"},
    {ScanMode::plane, P_GMC, "dir_plane together with gmc_max_shift / gmc_vectors: planes and compensation are not together yet"},
    {ScanMode::plane, P_PAIR, "dir_plane together with gmc_blob_cells / gmc_blob_sweep_levels: planes and the compensated blob scan are "
                              "not together yet"},
    {ScanMode::dir, P_BLOBS, "dir_allow together with min_blob_cells / blob_sweep_levels: direction and blobs are not together yet"},
    {ScanMode::dir, P_GMC, "dir_allow together with gmc_max_shift / gmc_vectors: direction and compensation are not together yet"},
    {ScanMode::dir, P_PAIR, "dir_allow together with gmc_blob_cells / gmc_blob_sweep_levels: direction and the compensated blob scan are "
                            "not together yet"}};

// `out`: a PipelineResult (or a test's struct with its input fields).  The fields that say "take the options" (-1, empty)
// receive the options' values, as run_scan_pipeline's callers read them afterwards.  Every conflict is answered here,
// before any decode.  Check order: blobs, gmc, pair, plane, dir, persist.
template <class Result>
inline PipelineModes resolve_pipeline(Result &out, const PipelineDefaults &opt, int clusters_needed) {
  PipelineModes m;
  auto refuse = [&m](std::string text) { m.error = std::move(text); return m; };
  const int floor_level = std::max(1, clusters_needed);
  if (out.sweep_levels.empty()) out.sweep_levels = opt.centre.sweep_levels;
  if (out.min_blob_cells < 0) out.min_blob_cells = opt.blob.min_blob_cells;
  if (out.blob_sweep_levels.empty()) out.blob_sweep_levels = opt.blob.sweep_levels;
  m.report_largest = !out.blob_sweep_levels.empty();
  const bool counts = out.keep_centres || opt.centre.keep || !out.sweep_levels.empty();   // the pipe's ONE count array is taken
  if (m.report_largest && counts) return refuse("blob_sweep_levels together with keep_centres / sweep_levels: the pipe has one count array");
  for (int level : out.blob_sweep_levels)
    if (level < floor_level) return refuse("blob sweep level " + std::to_string(level) + " is below max(1, CLUSTERS_NEEDED)");
  if (out.gmc_max_shift == -1) {
    out.gmc_max_shift = opt.gmc.max_shift < 0 ? -2 : opt.gmc.max_shift;
    out.gmc_min_share_q8 = opt.gmc.min_share_q8;
    out.gmc_vectors = out.gmc_vectors || opt.gmc.vectors;
  }
  m.gmc_on = out.gmc_max_shift >= 0;
  if (out.gmc_vectors && !m.gmc_on) return refuse("gmc_vectors without compensation (gmc_max_shift)");
  if (m.gmc_on && (out.gmc_max_shift > MTGPU_GMC_MAX_SHIFT || out.gmc_min_share_q8 < 0 || out.gmc_min_share_q8 > 256))
    return refuse("gmc_max_shift must be in [0, 127] and gmc_min_share_q8 in [0, 256]");
  unsigned asked = (out.min_blob_cells > 0 || m.report_largest ? P_BLOBS : 0u) | (m.gmc_on ? P_GMC : 0u);
  if (m.gmc_on)
    if (const char *t = not_together(PIPELINE_NOT_TOGETHER, ScanMode::gmc, asked)) return refuse(t);
  if (out.gmc_vectors && (counts || m.report_largest))
    return refuse("gmc_vectors together with keep_centres / sweep_levels / blob_sweep_levels: the pipe has one count array");
  // the compensated blob scan
  if (out.gmc_blob_cells == -1) {
    out.gmc_blob_cells = opt.pair.min_blob_cells;
    out.gmc_blob_max_shift = opt.pair.max_shift;
    out.gmc_blob_min_share_q8 = opt.pair.min_share_q8;
    if (out.gmc_blob_sweep_levels.empty()) out.gmc_blob_sweep_levels = opt.pair.sweep_levels;
  }
  m.pair_largest = !out.gmc_blob_sweep_levels.empty();
  m.pair_on = out.gmc_blob_cells > 0 || m.pair_largest;
  if (out.gmc_blob_cells < -1) return refuse("gmc_blob_cells is " + std::to_string(out.gmc_blob_cells));
  if (m.pair_on) {
    if (out.gmc_blob_max_shift < 0 || out.gmc_blob_max_shift > MTGPU_GMC_MAX_SHIFT || out.gmc_blob_min_share_q8 < 0 || out.gmc_blob_min_share_q8 > 256)
      return refuse("gmc_blob_max_shift must be in [0, 127] and gmc_blob_min_share_q8 in [0, 256]");
    if (const char *t = not_together(PIPELINE_NOT_TOGETHER, ScanMode::gmc_blobs, asked)) return refuse(t);
    if (m.pair_largest && counts) return refuse("gmc_blob_sweep_levels together with keep_centres / sweep_levels: the pipe has one count array");
    for (int level : out.gmc_blob_sweep_levels)
      if (level < floor_level) return refuse("gmc blob sweep level " + std::to_string(level) + " is below max(1, CLUSTERS_NEEDED)");
    asked |= P_PAIR;
  }
  // the direction byte and the direction plane
  if (out.dir_allow == -1) {
    out.dir_allow = opt.dir.allow < 0 ? -2 : opt.dir.allow;
    out.dir_sectors = out.dir_sectors || opt.dir.sectors;
  }
  m.dir_on = out.dir_allow >= 0;
  if (out.dir_allow < -2 || out.dir_allow > 255) return refuse("dir_allow is " + std::to_string(out.dir_allow) + ": want 0 .. 255, -1 or -2");
  if (out.dir_plane.empty()) out.dir_plane = opt.plane.plane;
  m.plane_on = !out.dir_plane.empty();
  if (out.dir_sectors && !m.dir_on && !m.plane_on) return refuse("dir_sectors without the direction mode (dir_allow)");
  if (m.dir_on) asked |= P_DIR;
  for (ScanMode x : {ScanMode::plane, ScanMode::dir}) {
    if (!(x == ScanMode::plane ? m.plane_on : m.dir_on)) continue;
    if (const char *t = not_together(PIPELINE_NOT_TOGETHER, x, asked)) return refuse(t);
    if (out.dir_sectors && counts) return refuse("dir_sectors together with keep_centres / sweep_levels: the pipe has one count array");
  }
  // temporal persistence: one pass per recording behind the scan
  if (out.min_run == -1) {
    out.min_run = opt.persist.min_run;
    out.max_dropout = opt.persist.max_dropout;
    out.reach = opt.persist.reach;
    if (out.run_sweep_levels.empty()) out.run_sweep_levels = opt.persist.sweep_levels;
  }
  if (out.min_run < -1) return refuse("min_run is " + std::to_string(out.min_run));
  m.persist_on = out.min_run > 1 || !out.run_sweep_levels.empty();
  if (m.persist_on) {
    const char *lv = !out.sweep_levels.empty() ? "sweep_levels" : m.report_largest ? "blob_sweep_levels" : m.pair_largest ? "gmc_blob_sweep_levels" : nullptr;
    if (lv)
      return refuse(std::string(out.min_run > 1 ? "min_run" : "run_sweep_levels") + " together with " + lv +
                    ": a level sweep under persistence needs one persistence pass per level, which is not built");
    if (out.reach >= 0 && out.min_blob_cells <= 0 && out.gmc_blob_cells <= 0)
      return refuse("reach without min_blob_cells / gmc_blob_cells: only a blob scan reports the box that reach compares");
    if (out.reach > 65535) return refuse("reach " + std::to_string(out.reach) + " outside [0,65535]");
  }
  m.keep_centres = counts || m.report_largest || out.gmc_vectors || m.pair_largest || out.dir_sectors;
  return m;
}

}  // namespace mtgpu_host
