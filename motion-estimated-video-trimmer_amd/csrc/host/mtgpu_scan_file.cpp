// mtgpu_scan_file — the scan + merge half of `motion_trim` on the GPU, reading extracted motion
// vectors from .mtmv containers instead of decoding with FFmpeg:
//   mtgpu_scan_file stream.mtmv [more.mtmv ...] [--threads T] [--streams S] [--outdir DIR] [--timestamps] [--summary]
//                   [--centres] [--sweep K1,K2,...] [--keep MASK.mtkeep] [--min-blob-cells N] [--sweep-blobs L1,L2,...]
//                   [--gmc] [--gmc-max-shift N] [--gmc-min-share-q8 Q] [--gmc-vectors]
//                   [--gmc-blobs N] [--gmc-blobs-max-shift S] [--gmc-blobs-min-share-q8 Q] [--sweep-gmc-blobs L1,L2,...]
//                   [--min-run N] [--max-dropout D] [--reach R] [--sweep-min-run L1,L2,...]
//                   [--allow LIST | --ignore LIST] [--dir-sectors] [--plane FILE.mtdir]
//   (--streams 0 / --threads 0: the reference's own sizing from PARALLEL_STREAMS / THREADS_PER_STREAM and the CPU limit)
// One file: like `motion_trim in out` (single ProcessingPipeline).  Several files: like
// `motion_trim in_dir out_dir` (BatchProcessor): S streams x T workers, jobs consumed by one
// thread (here: printed).  Configuration comes from the same environment variables as the
// reference (MV_THRESHOLD_SQ, VECTORS_NEEDED, CHUNK_DURATION_SEC, TARGET_FPS, ...).
// Prints one JSON object per input with a job: the FFmpegJob segment list (%.17g) + merge result.
// --centres: also "centres": [[pts, n], ...] — the centre count of every analysed frame (the `clusters` counter of
// motion_scanner.cpp:272-294 without its early return), sorted by pts.  --sweep 1,2,4,8: also "sweep": one entry per
// value k with the segments / do_cut / saved_pct / n_timestamps this tool prints when run with CLUSTERS_NEEDED=k —
// from the one scan.  Without the two options the output is unchanged.
// --keep MASK.mtkeep: ignore zones — every input is scanned under the keep mask of that file (mtgpu_host::load_keep;
// written by `python -m mvtrim_amd.zones --save-mask MASK.mtkeep`): check_frame's :282 gets one more term, so the
// segments are those of the recording without the ignored cells.  An input whose grid is not the mask's fails with the
// parser's message, the others go on.  The printed job gains "ignored_cells": N; without the option nothing changes.
// --min-blob-cells N: a minimum object size (include/mtgpu_pipe_blobs.h) — a frame has motion iff its centre count
// reaches CLUSTERS_NEEDED AND the largest 4-connected blob of its centres has at least N cells; under --keep both are
// taken on the masked cells.  --sweep-blobs 8,12,20: the pipes report every frame's largest blob; the job gains
// "largest": [[pts, n], ...] and "sweep_blobs": one entry per level L, in the format of "sweep", with the segments this
// tool prints when run with --min-blob-cells L — from the one scan.  A level must be at least max(1, CLUSTERS_NEEDED).
// --sweep-blobs together with --centres or --sweep is refused: a pipe has one count array.  Without the two options
// the output is unchanged.
// --gmc: global-motion compensation (include/mtgpu_pipe_gmc.h) — every frame is scanned against its own dominant
// vector, estimated within +-16 pixels and applied where half of the counted records agree; --gmc-max-shift N (0 .. 127)
// and --gmc-min-share-q8 Q (0 .. 256) change the two and each imply --gmc.  Under --keep the estimate counts only records
// of kept cells and the ignored cells are not active: a burnt-in clock neither votes for the vector nor shows as
// motion once the vector is subtracted.  --gmc-vectors (implies --gmc): the pipes report every frame's applied vector;
// the job gains "gmc": {"frames", "compensated_frames", "compensated_share" (of the frames scanned), "vectors":
// [[gx, gy, frames], ...] most frequent first}.  It combines with --keep, --centres and --sweep; --gmc-vectors does not
// combine with --centres or --sweep (a pipe has one count array); none of it combines with --min-blob-cells N > 0 or
// --sweep-blobs.  Without these options the output is unchanged.
// --gmc-blobs N: the compensated blob scan (include/mtgpu_pipe_gmc_blobs.h), a shaking camera in the rain — a frame has
// motion iff the centre count of its RESIDUAL vote reaches CLUSTERS_NEEDED AND the largest 4-connected blob of those
// centres has at least N cells; --gmc-blobs-max-shift S (0 .. 127) and --gmc-blobs-min-share-q8 Q (0 .. 256) set its
// compensation and are valid only next to --gmc-blobs or --sweep-gmc-blobs.  --sweep-gmc-blobs 3,8: the pipes report
// every frame's largest residual blob; the job gains "largest" and "sweep_gmc_blobs", in the format of "sweep_blobs",
// each level with the segments this tool prints when run with --gmc-blobs L.  It combines with --keep; --gmc-blobs
// combines with --centres / --sweep, --sweep-gmc-blobs does not (a pipe has one count array); none of it combines with
// --gmc, --gmc-max-shift, --gmc-min-share-q8, --gmc-vectors, --min-blob-cells N > 0 or --sweep-blobs.  Without these
// options the output is unchanged.
// --min-run N: temporal persistence (include/mtgpu_persist.h) — a motion frame counts only as one of a run of at least N
// motion frames; key frames (no side data) never break a run, --max-dropout D (default 0) quiet frames inside one are
// bridged, and with --reach R (no default; without it no boxes) a run also ends where the largest blob's box moves more
// than R cells — which needs --min-blob-cells N > 0 or --gmc-blobs N > 0 (include/mtgpu_pipe_boxes.h).  The rule is
// applied once per recording, after the scan, on every scanned frame in pts order: the result does not depend on
// CHUNK_DURATION_SEC or --threads.  Frames the TARGET_FPS skip drops are never scanned and are in no run.  The job gains
// "min_run", "max_dropout", "reach" (when given), "frames_before_persist" (the motion frames of the scan) and
// "persist_us"; "motion_frames", "segments" and the merge result are those of the kept frames.  --sweep-min-run 1,2,3:
// the job gains "runs": [[pts, run], ...] for every scanned frame and "sweep_min_run", in the format of "sweep_blobs",
// each level with the segments this tool prints when run with --min-run L — from the one scan and the one persistence
// pass.  --min-run N > 1 and --sweep-min-run do not combine with --sweep, --sweep-blobs or --sweep-gmc-blobs (a level
// sweep under persistence needs one persistence pass per level, which is not built); --max-dropout and --reach are valid
// only next to them.  --min-run 0 or 1 with nothing else prints exactly what no option prints.
// --allow LIST / --ignore LIST: the direction filter (include/mtgpu_pipe_dir.h) — a record votes only if the sector of
// dst - src is one of LIST (--allow) or none of LIST (--ignore); LIST holds sector names E,SE,S,SW,W,NW,N,NE or one
// decimal number 0 .. 255 (the byte of the sectors named); the two are mutually exclusive.  Under --keep the ignored cells are not
// active.  --dir-sectors (implies the mode, with every sector allowed when neither list is given): the pipes report every
// frame's sector word; the job gains "dir": {"allow", "frames" (scanned frames with a counting moving record),
// "present": [8] (frames in which sector k has a counting record), "dominant": [8] (frames whose strongest sector is
// k)}, counted under --keep where it is given and whatever the lists say.  It combines with --keep, --centres, --sweep,
// --min-run, --max-dropout and --sweep-min-run; --dir-sectors does not combine with --centres or --sweep (a pipe has one
// count array); none of it combines with the --gmc family, --min-blob-cells N > 0, --sweep-blobs, the --gmc-blobs family
// or --reach.  Without these options the output is unchanged.
// --plane FILE.mtdir: a direction plane (include/mtgpu_pipe_lanes.h) — one allow byte per grid cell where --allow has one
// for the whole picture: a record votes only if its destination cell's byte has the bit of its sector
// (mtgpu_host::load_plane; `python -m mvtrim_amd.lanes --learn --save-plane` writes such a file).  Loaded per input
// against that input's grid, as --keep is; a mismatch is the loader's message with the line named.  It combines with
// --keep, --centres, --sweep, --min-run and --dir-sectors (the "dir" object then carries "plane": "<path>" in place of
// "allow"); it does not combine with --allow / --ignore (one rule at two granularities), the --gmc family, the blob
// options or --reach.
// --summary (several files): one more line {"batch_summary": ...} — frames scanned, wall time, worker-time
// breakdown and what the S x T workers held (contexts, pipes, HIP streams, pinned / device bytes).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <strings.h>   // strncasecmp

#include "mtgpu_host.hpp"

using namespace mtgpu_host;

// --repeat N (rate measurements only): the input presented as N back-to-back copies of itself — a
// long video whose MV bytes stay cache-resident, like side data a decoder thread has just written,
// instead of 10+ GB streamed from the page cache.
class RepeatSource : public FrameSource {
  const MtmvFile &f_;
  uint64_t reps_, pos_ = 0;
  int64_t period_;     // ticks per copy
 public:
  RepeatSource(const MtmvFile &f, uint64_t reps) : f_(f), reps_(reps) {
    period_ = (int64_t)std::llround(f.hdr->duration * (double)f.hdr->tb_den / (double)f.hdr->tb_num);
  }
  int width() const override { return (int)f_.hdr->width; }
  int height() const override { return (int)f_.hdr->height; }
  double duration() const override { return f_.hdr->duration * (double)reps_; }
  double fps() const override { return f_.hdr->fps; }
  double time_base() const override { return (double)f_.hdr->tb_num / (double)f_.hdr->tb_den; }
  void seek(double seconds) override {
    const int64_t target = static_cast<int64_t>(seconds / time_base());
    uint64_t rep = period_ > 0 ? (uint64_t)(target / period_) : 0;
    if (rep >= reps_) rep = reps_ - 1;
    const int64_t local = target - (int64_t)rep * period_;
    uint64_t key = 0;
    for (uint64_t i = 0; i < f_.hdr->n_frames && f_.frames[i].pts <= local; ++i)
      if (f_.frames[i].key) key = i;
    pos_ = rep * f_.hdr->n_frames + key;
  }
  bool next(Frame &fr) override {
    const uint64_t n = f_.hdr->n_frames;
    if (n == 0 || pos_ >= reps_ * n) return false;
    const uint64_t rep = pos_ / n;
    const MtmvFrameRec &r = f_.frames[pos_ % n];
    ++pos_;
    fr.pts = r.pts + (int64_t)rep * period_;
    fr.has_side_data = r.has_sd != 0;
    fr.mv = r.has_sd ? f_.records + 40ull * r.rec_off : nullptr;
    fr.mv_bytes = r.has_sd ? 40ull * r.n_rec : 0;
    return true;
  }
};

static bool g_summary = false;    // --summary
static bool g_print_ts = false;   // --timestamps: also print the pooled motion timestamps, sorted (%.17g)
static bool g_print_centres = false;   // --centres
static std::string g_keep_path;        // --keep
static bool g_print_largest = false;   // --sweep-blobs
static bool g_print_gmc = false;       // --gmc-vectors
static const char *g_pair_opt = nullptr;        // the first of --gmc-blobs N > 0 / --sweep-gmc-blobs given
static const char *g_pair_param_opt = nullptr;  // the first of --gmc-blobs-max-shift / --gmc-blobs-min-share-q8 given
static const char *g_gmc_opt = nullptr;         // the first option of the --gmc family given
static const char *g_persist_param_opt = nullptr;   // the first of --max-dropout / --reach given
static bool g_sweep_opt = false;                    // --sweep given
static const char *g_dir_opt = nullptr;             // the first of --allow / --ignore / --dir-sectors given
static const char *g_dir_list_opt = nullptr;        // --allow or --ignore, whichever was given
static bool g_print_dir = false;                    // --dir-sectors
static std::string g_plane_path;                    // --plane

// LIST of --allow / --ignore: sector names E,SE,S,SW,W,NW,N,NE (any case) or one decimal number 0 .. 255 -> the byte of
// the sectors named.
static bool parse_sector_list(const char *text, int *byte) {
  static const char *const names[8] = {"E", "SE", "S", "SW", "W", "NW", "N", "NE"};
  if (!text || !*text) return false;
  if (*text >= '0' && *text <= '9') {
    char *end = nullptr;
    const long v = std::strtol(text, &end, 10);    // decimal only: "010" is ten, "0x11" is refused
    if (*end || v < 0 || v > 255) return false;
    *byte = (int)v;
    return true;
  }
  int b = 0;
  for (const char *q = text; *q;) {
    const char *e = std::strchr(q, ',');
    const size_t n = e ? (size_t)(e - q) : std::strlen(q);
    int k = -1;
    for (int j = 0; j < 8; ++j)
      if (std::strlen(names[j]) == n && !strncasecmp(q, names[j], n)) k = j;
    if (k < 0 || (e && !e[1])) return false;
    b |= 1 << k;
    q = e ? e + 1 : q + n;
  }
  *byte = b;
  return true;
}

// The keep mask of g_keep_path for a width x height input; throws with load_keep's message (the line is named) when the
// file is malformed or made for another grid.
static std::vector<uint64_t> keep_for_size(int width, int height) {
  Config::load_all();
  mt_scan_params p;
  if (mtgpu_params_from_config(&p, width, height, Config::mv_threshold_sq(), Config::block_size(), Config::block_shift(),
                               Config::vectors_needed(), Config::clusters_needed(), Config::vertical_mask()) != MT_OK)
    throw std::runtime_error(mtgpu_last_error());
  std::vector<uint64_t> words;
  std::string err;
  if (!load_keep(g_keep_path, p.grid_w, p.grid_h, words, err)) throw std::runtime_error("--keep: " + err);
  return words;
}

// The direction plane of g_plane_path for a width x height input; throws with load_plane's message (the line is named)
// when the file is malformed or made for another grid.
static std::vector<uint8_t> plane_for_size(int width, int height) {
  Config::load_all();
  mt_scan_params p;
  if (mtgpu_params_from_config(&p, width, height, Config::mv_threshold_sq(), Config::block_size(), Config::block_shift(),
                               Config::vectors_needed(), Config::clusters_needed(), Config::vertical_mask()) != MT_OK)
    throw std::runtime_error(mtgpu_last_error());
  std::vector<uint8_t> bytes;
  std::string err;
  if (!load_plane(g_plane_path, p.grid_w, p.grid_h, bytes, err)) throw std::runtime_error("--plane: " + err);
  return bytes;
}

static unsigned long long ignored_cells(const std::vector<uint64_t> &keep, int width, int height) {
  mt_scan_params p;
  if (mtgpu_params_from_config(&p, width, height, Config::mv_threshold_sq(), Config::block_size(), Config::block_shift(),
                               Config::vectors_needed(), Config::clusters_needed(), Config::vertical_mask()) != MT_OK)
    return 0;
  unsigned long long kept = 0;
  for (uint64_t w : keep) kept += (unsigned long long)__builtin_popcountll(w);
  return (unsigned long long)p.grid_w * (unsigned long long)p.grid_h - kept;
}

static void print_job(const std::string &input, const PipelineResult &r, const std::vector<mt_segment> &segs, int width = 0,
                      int height = 0) {
  std::printf("{\"input\": \"%s\", \"chunks\": %d, \"threads\": %d, \"frames_scanned\": %llu, \"motion_frames\": %zu, \"n_timestamps\": %llu, "
              "\"do_cut\": %d, \"time_removed\": %.17g, \"saved_pct\": %.17g, \"seek_us\": %ld, "
              "\"decode_us\": %ld, \"analyze_us\": %ld, \"init_us\": %ld, \"scan_wall_us\": %ld, \"scan_work_us\": %ld, "
              "\"copy_us\": %ld, \"submit_us\": %ld, \"wait_us\": %ld, \"segments\": [",
              input.c_str(), r.chunks, r.threads, (unsigned long long)r.frames_scanned, r.motion_frames,
              (unsigned long long)r.merge.n_timestamps,
              r.merge.do_cut, r.merge.time_removed, r.merge.saved_pct, r.seek_us, r.decode_us, r.analyze_us, r.init_us,
              r.scan_wall_us, r.scan_work_us, r.copy_us, r.submit_us, r.wait_us);
  for (size_t i = 0; i < segs.size(); ++i)
    std::printf("%s[%.17g, %.17g]", i ? ", " : "", segs[i].start, segs[i].end);
  std::printf("]");
  if (!g_keep_path.empty()) std::printf(", \"ignored_cells\": %llu", ignored_cells(r.keep, width, height));
  if (g_print_ts) {
    std::vector<double> ts = r.timestamps;
    std::sort(ts.begin(), ts.end());
    std::printf(", \"timestamps\": [");
    for (size_t i = 0; i < ts.size(); ++i) std::printf("%s%.17g", i ? ", " : "", ts[i]);
    std::printf("]");
  }
  if (g_print_centres) {
    std::printf(", \"centres\": [");
    for (size_t i = 0; i < r.centres.size(); ++i) std::printf("%s[%.17g, %u]", i ? ", " : "", r.centres[i].first, r.centres[i].second);
    std::printf("]");
  }
  if (g_print_largest || !gmc_blob_options().sweep_levels.empty()) {
    std::printf(", \"largest\": [");
    for (size_t i = 0; i < r.centres.size(); ++i) std::printf("%s[%.17g, %u]", i ? ", " : "", r.centres[i].first, r.centres[i].second);
    std::printf("]");
  }
  const auto print_sweep = [](const char *name, const char *level, const std::vector<PipelineResult::SweepEntry> &sweep) {
    std::printf(", \"%s\": [", name);
    for (size_t k = 0; k < sweep.size(); ++k) {
      const PipelineResult::SweepEntry &e = sweep[k];
      std::printf("%s{\"%s\": %d, \"segments\": [", k ? ", " : "", level, e.clusters_needed);
      for (size_t i = 0; i < e.segments.size(); ++i)
        std::printf("%s[%.17g, %.17g]", i ? ", " : "", e.segments[i].start, e.segments[i].end);
      std::printf("], \"do_cut\": %d, \"saved_pct\": %.17g, \"n_timestamps\": %llu}", e.merge.do_cut, e.merge.saved_pct,
                  (unsigned long long)e.merge.n_timestamps);
    }
    std::printf("]");
  };
  if (g_print_gmc) {
    std::printf(", \"gmc\": {\"frames\": %zu, \"compensated_frames\": %llu, \"compensated_share\": %.17g, \"vectors\": [", r.centres.size(),
                (unsigned long long)r.gmc_moved_frames, r.centres.empty() ? 0.0 : (double)r.gmc_moved_frames / (double)r.centres.size());
    for (size_t i = 0; i < r.gmc_top.size(); ++i)
      std::printf("%s[%d, %d, %llu]", i ? ", " : "", r.gmc_top[i].gx, r.gmc_top[i].gy, (unsigned long long)r.gmc_top[i].frames);
    std::printf("]}");
  }
  if (g_print_dir) {
    if (!g_plane_path.empty())
      std::printf(", \"dir\": {\"plane\": \"%s\", \"frames\": %llu, \"present\": [", g_plane_path.c_str(), (unsigned long long)r.dir_frames);
    else
      std::printf(", \"dir\": {\"allow\": %d, \"frames\": %llu, \"present\": [", r.dir_allow, (unsigned long long)r.dir_frames);
    for (int k = 0; k < 8; ++k) std::printf("%s%llu", k ? ", " : "", (unsigned long long)r.dir_present_frames[k]);
    std::printf("], \"dominant\": [");
    for (int k = 0; k < 8; ++k) std::printf("%s%llu", k ? ", " : "", (unsigned long long)r.dir_dominant_frames[k]);
    std::printf("]}");
  }
  if (!r.sweep.empty()) print_sweep("sweep", "clusters_needed", r.sweep);
  if (!r.blob_sweep.empty()) print_sweep("sweep_blobs", "min_blob_cells", r.blob_sweep);
  if (!r.gmc_blob_sweep.empty()) print_sweep("sweep_gmc_blobs", "min_blob_cells", r.gmc_blob_sweep);
  if (r.min_run > 1 || !r.run_sweep_levels.empty()) {
    std::printf(", \"min_run\": %d, \"max_dropout\": %u", std::max(1, r.min_run), (unsigned)r.max_dropout);
    if (r.reach >= 0) std::printf(", \"reach\": %d", r.reach);
    std::printf(", \"frames_before_persist\": %zu, \"persist_us\": %ld", r.frames_before_persist, r.persist_us);
  }
  if (!r.run_sweep_levels.empty()) {
    std::printf(", \"runs\": [");
    for (size_t i = 0; i < r.runs.size(); ++i) std::printf("%s[%.17g, %u]", i ? ", " : "", r.runs[i].first, r.runs[i].second);
    std::printf("]");
    print_sweep("sweep_min_run", "min_run", r.run_sweep);
  }
  std::printf("}\n");
  std::fflush(stdout);
}

int main(int argc, char **argv) {
  std::vector<std::string> files;
  int threads = 4, streams = 2;
  long repeat = 1;
  std::string outdir = ".";
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--threads") && i + 1 < argc) threads = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--streams") && i + 1 < argc) streams = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--outdir") && i + 1 < argc) outdir = argv[++i];
    else if (!std::strcmp(argv[i], "--timestamps")) g_print_ts = true;
    else if (!std::strcmp(argv[i], "--summary")) g_summary = true;
    else if (!std::strcmp(argv[i], "--centres")) { g_print_centres = true; centre_options().keep = true; }
    else if (!std::strcmp(argv[i], "--sweep") && i + 1 < argc) {
      g_sweep_opt = true;
      for (const char *q = argv[++i]; *q;) {
        char *end = nullptr;
        const long v = std::strtol(q, &end, 10);
        if (end == q) { std::fprintf(stderr, "error: --sweep takes a comma-separated list of integers\n"); return 2; }
        centre_options().sweep_levels.push_back((int)v);
        q = (*end == ',') ? end + 1 : end;
        if (*end && *end != ',') { std::fprintf(stderr, "error: --sweep takes a comma-separated list of integers\n"); return 2; }
      }
    }
    else if (!std::strcmp(argv[i], "--repeat") && i + 1 < argc) repeat = std::atol(argv[++i]);
    else if (!std::strcmp(argv[i], "--keep")) {
      if (i + 1 >= argc) { std::fprintf(stderr, "error: --keep takes the path of a .mtkeep file\n"); return 2; }
      g_keep_path = argv[++i];
    }
    else if (!std::strcmp(argv[i], "--plane")) {
      if (i + 1 >= argc) { std::fprintf(stderr, "error: --plane takes the path of a .mtdir file\n"); return 2; }
      g_plane_path = argv[++i];
    }
    else if (!std::strcmp(argv[i], "--min-blob-cells")) {
      char *end = nullptr;
      const long v = i + 1 < argc ? std::strtol(argv[i + 1], &end, 10) : -1;
      if (i + 1 >= argc || end == argv[i + 1] || *end || v < 0 || v > 0x7fffffffL) {
        std::fprintf(stderr, "error: --min-blob-cells takes a cell count >= 0\n");
        return 2;
      }
      ++i;
      blob_options().min_blob_cells = (int)v;
    }
    else if (!std::strcmp(argv[i], "--sweep-blobs")) {
      const char *q = i + 1 < argc ? argv[++i] : "";
      if (!*q) { std::fprintf(stderr, "error: --sweep-blobs takes a comma-separated list of integers\n"); return 2; }
      while (*q) {
        char *end = nullptr;
        const long v = std::strtol(q, &end, 10);
        if (end == q || (*end && (*end != ',' || !end[1])) || v > 0x7fffffffL || v < -0x7fffffffL) {
          std::fprintf(stderr, "error: --sweep-blobs takes a comma-separated list of integers\n");
          return 2;
        }
        blob_options().sweep_levels.push_back((int)v);
        q = *end ? end + 1 : end;
      }
      g_print_largest = true;
    }
    else if (!std::strcmp(argv[i], "--gmc-blobs")) {
      char *end = nullptr;
      const long v = i + 1 < argc ? std::strtol(argv[i + 1], &end, 10) : -1;
      if (i + 1 >= argc || end == argv[i + 1] || *end || v < 0 || v > 0x7fffffffL) {
        std::fprintf(stderr, "error: --gmc-blobs takes a cell count >= 0\n");
        return 2;
      }
      ++i;
      gmc_blob_options().min_blob_cells = (int)v;
      if (v > 0 && !g_pair_opt) g_pair_opt = "--gmc-blobs";
    }
    else if (!std::strcmp(argv[i], "--sweep-gmc-blobs")) {
      const char *q = i + 1 < argc ? argv[++i] : "";
      if (!*q) { std::fprintf(stderr, "error: --sweep-gmc-blobs takes a comma-separated list of integers\n"); return 2; }
      while (*q) {
        char *end = nullptr;
        const long v = std::strtol(q, &end, 10);
        if (end == q || (*end && (*end != ',' || !end[1])) || v > 0x7fffffffL || v < -0x7fffffffL) {
          std::fprintf(stderr, "error: --sweep-gmc-blobs takes a comma-separated list of integers\n");
          return 2;
        }
        gmc_blob_options().sweep_levels.push_back((int)v);
        q = *end ? end + 1 : end;
      }
      if (!g_pair_opt) g_pair_opt = "--sweep-gmc-blobs";
    }
    else if (!std::strcmp(argv[i], "--gmc-blobs-max-shift") || !std::strcmp(argv[i], "--gmc-blobs-min-share-q8")) {
      const bool shift = !std::strcmp(argv[i], "--gmc-blobs-max-shift");
      const long hi = shift ? MTGPU_GMC_MAX_SHIFT : 256;
      char *end = nullptr;
      const long v = i + 1 < argc ? std::strtol(argv[i + 1], &end, 10) : -1;
      if (i + 1 >= argc || end == argv[i + 1] || *end || v < 0 || v > hi) {
        std::fprintf(stderr, "error: %s takes an integer in [0, %ld]\n", argv[i], hi);
        return 2;
      }
      if (!g_pair_param_opt) g_pair_param_opt = argv[i];
      ++i;
      (shift ? gmc_blob_options().max_shift : gmc_blob_options().min_share_q8) = (int)v;
    }
    else if (!std::strcmp(argv[i], "--gmc")) {
      if (!g_gmc_opt) g_gmc_opt = argv[i];
      if (gmc_options().max_shift < 0) gmc_options().max_shift = MTGPU_GMC_DEFAULT_MAX_SHIFT;
    }
    else if (!std::strcmp(argv[i], "--gmc-vectors")) {
      if (!g_gmc_opt) g_gmc_opt = argv[i];
      if (gmc_options().max_shift < 0) gmc_options().max_shift = MTGPU_GMC_DEFAULT_MAX_SHIFT;
      gmc_options().vectors = true;
      g_print_gmc = true;
    }
    else if (!std::strcmp(argv[i], "--gmc-max-shift") || !std::strcmp(argv[i], "--gmc-min-share-q8")) {
      const bool shift = !std::strcmp(argv[i], "--gmc-max-shift");
      const long hi = shift ? MTGPU_GMC_MAX_SHIFT : 256;
      char *end = nullptr;
      const long v = i + 1 < argc ? std::strtol(argv[i + 1], &end, 10) : -1;
      if (i + 1 >= argc || end == argv[i + 1] || *end || v < 0 || v > hi) {
        std::fprintf(stderr, "error: %s takes an integer in [0, %ld]\n", argv[i], hi);
        return 2;
      }
      if (!g_gmc_opt) g_gmc_opt = argv[i];
      ++i;
      if (shift) gmc_options().max_shift = (int)v;
      else {
        gmc_options().min_share_q8 = (int)v;
        if (gmc_options().max_shift < 0) gmc_options().max_shift = MTGPU_GMC_DEFAULT_MAX_SHIFT;
      }
    }
    else if (!std::strcmp(argv[i], "--min-run") || !std::strcmp(argv[i], "--max-dropout") || !std::strcmp(argv[i], "--reach")) {
      const bool run = !std::strcmp(argv[i], "--min-run"), drop = !std::strcmp(argv[i], "--max-dropout");
      const long long hi = run ? 0x7fffffffLL : drop ? 0xffffffffLL : 65535LL;
      char *end = nullptr;
      const long long v = i + 1 < argc ? std::strtoll(argv[i + 1], &end, 10) : -1;
      if (i + 1 >= argc || end == argv[i + 1] || *end || v < 0 || v > hi) {
        std::fprintf(stderr, "error: %s takes an integer in [0, %lld]\n", argv[i], hi);
        return 2;
      }
      if (!run && !g_persist_param_opt) g_persist_param_opt = argv[i];
      ++i;
      if (run) persist_options().min_run = (int)v;
      else if (drop) persist_options().max_dropout = (uint32_t)v;
      else persist_options().reach = (int)v;
    }
    else if (!std::strcmp(argv[i], "--allow") || !std::strcmp(argv[i], "--ignore")) {
      const bool allow_opt = !std::strcmp(argv[i], "--allow");
      int byte = -1;
      if (i + 1 >= argc || !parse_sector_list(argv[i + 1], &byte)) {
        std::fprintf(stderr, "error: %s takes a comma-separated list of sector names (E,SE,S,SW,W,NW,N,NE) or one decimal number in [0, 255]\n", argv[i]);
        return 2;
      }
      if (g_dir_list_opt && std::strcmp(g_dir_list_opt, argv[i])) {
        std::fprintf(stderr, "error: --allow cannot be combined with --ignore: give the sectors that vote or the sectors that do not\n");
        return 2;
      }
      g_dir_list_opt = argv[i];
      if (!g_dir_opt) g_dir_opt = argv[i];
      ++i;
      dir_options().allow = allow_opt ? byte : (~byte & 0xff);
    }
    else if (!std::strcmp(argv[i], "--dir-sectors")) {
      if (!g_dir_opt) g_dir_opt = argv[i];
      g_print_dir = true;
      dir_options().sectors = true;
    }
    else if (!std::strcmp(argv[i], "--sweep-min-run")) {
      const char *q = i + 1 < argc ? argv[++i] : "";
      if (!*q) { std::fprintf(stderr, "error: --sweep-min-run takes a comma-separated list of integers\n"); return 2; }
      while (*q) {
        char *end = nullptr;
        const long v = std::strtol(q, &end, 10);
        if (end == q || (*end && (*end != ',' || !end[1])) || v > 0x7fffffffL || v < 0) {
          std::fprintf(stderr, "error: --sweep-min-run takes a comma-separated list of integers >= 0\n");
          return 2;
        }
        persist_options().sweep_levels.push_back((int)v);
        q = *end ? end + 1 : end;
      }
    }
    else files.push_back(argv[i]);
  }
  // --dir-sectors alone: the mode with every sector allowed
  if (g_print_dir && dir_options().allow < 0 && g_plane_path.empty()) dir_options().allow = 0xff;
  // the first option that stands for blobs or compensation: what neither a direction plane nor the direction filter goes with
  const char *const other = g_gmc_opt ? g_gmc_opt : g_pair_opt ? g_pair_opt : g_pair_param_opt ? g_pair_param_opt :
                            g_print_largest ? "--sweep-blobs" : blob_options().min_blob_cells > 0 ? "--min-blob-cells" :
                            persist_options().reach >= 0 ? "--reach" : nullptr;
  // what a direction plane cannot be combined with: answered here, before any device call and before the plane is read
  if (!g_plane_path.empty()) {
    if (g_dir_list_opt) {
      std::fprintf(stderr, "error: --plane cannot be combined with %s: a plane and the allow byte are one rule at two granularities\n", g_dir_list_opt);
      return 2;
    }
    if (other) {
      std::fprintf(stderr, "error: --plane cannot be combined with %s: planes are not together with blobs or compensation yet\n", other);
      return 2;
    }
  }
  // what the direction filter cannot be combined with: answered here, before any device call
  if (g_dir_opt) {
    if (other) {
      std::fprintf(stderr, "error: %s cannot be combined with %s: direction is not together with blobs or compensation yet\n", g_dir_opt, other);
      return 2;
    }
    if (g_print_dir && (g_print_centres || !centre_options().sweep_levels.empty())) {
      std::fprintf(stderr, "error: --dir-sectors cannot be combined with %s: a pipe has one count array\n", g_print_centres ? "--centres" : "--sweep");
      return 2;
    }
  }
  // what persistence cannot be combined with: answered here, before any device call
  {
    const PersistOptions &po = persist_options();
    const bool persist_on = po.min_run > 1 || !po.sweep_levels.empty();
    const char *mine = po.min_run > 1 ? "--min-run" : "--sweep-min-run";
    if (g_persist_param_opt && !persist_on) {
      std::fprintf(stderr, "error: %s is valid only next to --min-run N > 1 or --sweep-min-run\n", g_persist_param_opt);
      return 2;
    }
    if (persist_on) {
      const char *other = g_sweep_opt ? "--sweep" : g_print_largest ? "--sweep-blobs" : !gmc_blob_options().sweep_levels.empty() ? "--sweep-gmc-blobs" : nullptr;
      if (other) {
        std::fprintf(stderr, "error: %s cannot be combined with %s: a level sweep under persistence needs one persistence pass per "
                     "level, which is not built\n", mine, other);
        return 2;
      }
      if (po.reach >= 0 && blob_options().min_blob_cells <= 0 && gmc_blob_options().min_blob_cells <= 0) {
        std::fprintf(stderr, "error: --reach needs --min-blob-cells N > 0 or --gmc-blobs N > 0: only a blob scan reports the box that "
                     "--reach compares\n");
        return 2;
      }
    }
  }
  // what the compensated blob scan cannot be combined with: answered here, before any device call
  if (g_pair_param_opt && !g_pair_opt) {
    std::fprintf(stderr, "error: %s is valid only next to --gmc-blobs or --sweep-gmc-blobs\n", g_pair_param_opt);
    return 2;
  }
  if (g_pair_opt) {
    if (g_gmc_opt) {
      std::fprintf(stderr, "error: %s cannot be combined with %s: the compensated blob scan has its own compensation "
                   "(--gmc-blobs-max-shift, --gmc-blobs-min-share-q8)\n", g_pair_opt, g_gmc_opt);
      return 2;
    }
    if (blob_options().min_blob_cells > 0 || g_print_largest) {
      std::fprintf(stderr, "error: %s cannot be combined with %s: the compensated blob scan has its own minimum blob size\n",
                   g_pair_opt, g_print_largest ? "--sweep-blobs" : "--min-blob-cells");
      return 2;
    }
    if (!gmc_blob_options().sweep_levels.empty()) {
      if (g_print_centres || !centre_options().sweep_levels.empty()) {
        std::fprintf(stderr, "error: --sweep-gmc-blobs cannot be combined with --centres or --sweep: a pipe has one count array\n");
        return 2;
      }
      int need = 1;
      try { need = std::max(1, Config::clusters_needed()); }
      catch (const std::exception &e) { std::fprintf(stderr, "error: configuration: %s\n", e.what()); return 1; }
      for (int level : gmc_blob_options().sweep_levels)
        if (level < need) {
          std::fprintf(stderr, "error: --sweep-gmc-blobs level %d is below max(1, CLUSTERS_NEEDED) = %d\n", level, need);
          return 2;
        }
    }
  }
  // what compensation cannot be combined with: answered here, before any device call
  if (gmc_options().max_shift >= 0) {
    if (blob_options().min_blob_cells > 0 || g_print_largest) {
      std::fprintf(stderr, "error: --gmc cannot be combined with --min-blob-cells or --sweep-blobs: compensation and blobs are not together yet\n");
      return 2;
    }
    if (g_print_gmc && (g_print_centres || !centre_options().sweep_levels.empty())) {
      std::fprintf(stderr, "error: --gmc-vectors cannot be combined with --centres or --sweep: a pipe has one count array\n");
      return 2;
    }
  }
  // what the blob options cannot be combined with: answered here, before any device call
  if (g_print_largest) {
    if (g_print_centres || !centre_options().sweep_levels.empty()) {
      std::fprintf(stderr, "error: --sweep-blobs cannot be combined with --centres or --sweep: a pipe has one count array\n");
      return 2;
    }
    int need = 1;
    try { need = std::max(1, Config::clusters_needed()); }
    catch (const std::exception &e) { std::fprintf(stderr, "error: configuration: %s\n", e.what()); return 1; }
    for (int level : blob_options().sweep_levels)
      if (level < need) {
        std::fprintf(stderr, "error: --sweep-blobs level %d is below max(1, CLUSTERS_NEEDED) = %d\n", level, need);
        return 2;
      }
  }
  // --streams 0 / --threads 0: sized from the CPU budget, the devices and the number of videos (default_batch_sizing,
  // mtgpu_host.hpp — deliberately not the reference's CPU-only rule, src/system.cpp:186-197); PARALLEL_STREAMS /
  // THREADS_PER_STREAM are honoured as in the reference (config.hpp:138-141, 165-168)
  if (streams <= 0 || threads <= 0) {
    try {
      const BatchSizing z = default_batch_sizing((int)files.size(), mtgpu_device_count(), cpu_budget(),
                                                 streams > 0 ? streams : Config::parallel_streams(),
                                                 threads > 0 ? threads : Config::threads_per_stream());
      if (streams <= 0) streams = z.streams;
      if (threads <= 0) threads = z.threads;
    } catch (const std::exception &e) {
      std::fprintf(stderr, "error: configuration: %s\n", e.what());
      return 1;
    }
  }
  if (files.empty()) {
    std::fprintf(stderr, "usage: %s stream.mtmv [more.mtmv ...] [--threads T] [--streams S] [--outdir DIR]\n", argv[0]);
    return 2;
  }
  try {
    if (files.size() == 1) {
      MtmvFile file(files[0]);
      PipelineResult r;
      if (!g_keep_path.empty()) r.keep = keep_for_size((int)file.hdr->width, (int)file.hdr->height);
      if (!g_plane_path.empty()) r.dir_plane = plane_for_size((int)file.hdr->width, (int)file.hdr->height);
      int rc = run_scan_pipeline([&]() -> std::unique_ptr<FrameSource> {
        if (repeat > 1) return std::unique_ptr<FrameSource>(new RepeatSource(file, (uint64_t)repeat));
        return std::unique_ptr<FrameSource>(new MtmvSource(file));
      }, threads, r);
      if (rc != 0) { std::fprintf(stderr, "error: %s\n", r.error.c_str()); return 1; }
      print_job(files[0], r, r.segments, (int)file.hdr->width, (int)file.hdr->height);
      return 0;
    }
    // batch: mmaps are shared by the workers of a stream and kept until the end
    std::mutex mm;
    std::map<std::string, std::shared_ptr<MtmvFile>> open_files;
    auto open_source = [&](const std::string &path) {
      std::shared_ptr<MtmvFile> f = std::make_shared<MtmvFile>(path);   // mapped (and pre-faulted) outside the lock:
      { std::lock_guard<std::mutex> l(mm); open_files[path] = f; }       // 64 streams open their files concurrently
      return [f, repeat]() -> std::unique_ptr<FrameSource> {
        if (repeat > 1) return std::unique_ptr<FrameSource>(new RepeatSource(*f, (uint64_t)repeat));
        return std::unique_ptr<FrameSource>(new MtmvSource(*f));
      };
    };
    auto size_of = [&](const std::string &path, int &w, int &h) {
      std::lock_guard<std::mutex> l(mm);
      const auto it = open_files.find(path);
      w = it == open_files.end() ? 0 : (int)it->second->hdr->width;
      h = it == open_files.end() ? 0 : (int)it->second->hdr->height;
    };
    auto keep_for = [&](const std::string &path) -> std::vector<uint64_t> {
      if (g_keep_path.empty()) return {};
      int w = 0, h = 0;
      size_of(path, w, h);
      return keep_for_size(w, h);
    };
    auto plane_for = [&](const std::string &path) -> std::vector<uint8_t> {
      if (g_plane_path.empty()) return {};
      int w = 0, h = 0;
      size_of(path, w, h);
      return plane_for_size(w, h);
    };
    JobQueue jobs;
    std::vector<std::string> errors;
    int failed = 0;
    BatchSummary sum;
    std::thread producer([&] { failed = process_batch(files, outdir, streams, threads, open_source, jobs, &errors, &sum, keep_for, plane_for); });
    ScanJob job;                                   // the single consumer (batch_processor.cpp:138-150)
    while (jobs.pop(job)) {
      int w = 0, h = 0;
      size_of(job.input_path, w, h);
      print_job(job.input_path, job.result, job.segments, w, h);
    }
    producer.join();
    if (g_summary) {
      const Resources &h = sum.held;
      std::printf("{\"batch_summary\": {\"streams\": %d, \"threads_per_stream\": %d, \"videos\": %zu, \"jobs\": %zu, "
                  "\"failed\": %zu, \"frames_scanned\": %llu, \"wall_us\": %ld, \"scan_wall_us\": %ld, \"scan_window_us\": %ld, \"init_us\": %ld, \"decode_us\": %ld, "
                  "\"analyze_us\": %ld, \"copy_us\": %ld, \"submit_us\": %ld, \"wait_us\": %ld, \"cpu_user_us\": %ld, \"cpu_sys_us\": %ld, \"worker_cpu_us\": %ld, \"gate_wait_us\": %ld, \"gate_tokens\": %d, \"cpu_window\": %d, \"cpu_window_first\": %d, "
                  "\"held\": {\"contexts\": %llu, \"pipes\": %llu, \"hip_streams\": %llu, \"hip_events\": %llu, "
                  "\"mem_pools\": %llu, \"pinned_bytes\": %llu, \"device_bytes\": %llu, \"scratch_pool_high_bytes\": %llu, "
                  "\"submits\": %llu, \"ctx_create_us\": %llu, \"pipe_create_us\": %llu, \"pipe_rebuilds\": %llu, \"pin_us\": %llu, \"pinned_batches\": %llu}}}\n",
                  sum.streams, sum.threads_per_stream, sum.videos, sum.jobs, sum.failed,
                  (unsigned long long)sum.frames_scanned, sum.wall_us, sum.scan_wall_us, sum.scan_window_us, sum.init_us, sum.decode_us, sum.analyze_us,
                  sum.copy_us, sum.submit_us, sum.wait_us, sum.cpu_user_us, sum.cpu_sys_us, sum.worker_cpu_us, sum.gate_wait_us, sum.gate_tokens, sum.cpu_window, sum.cpu_window_first, (unsigned long long)h.contexts, (unsigned long long)h.pipes,
                  (unsigned long long)h.hip_streams, (unsigned long long)h.hip_events, (unsigned long long)h.mem_pools,
                  (unsigned long long)h.pinned_bytes, (unsigned long long)h.device_bytes,
                  (unsigned long long)h.pool_reserved_high, (unsigned long long)h.submits,
                  (unsigned long long)h.ctx_create_us, (unsigned long long)h.pipe_create_us,
                  (unsigned long long)h.pipe_rebuilds, (unsigned long long)h.pin_us, (unsigned long long)h.pinned_batches);
      std::fflush(stdout);
    }
    for (auto &e : errors) std::fprintf(stderr, "error: %s\n", e.c_str());
    return failed ? 1 : 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
