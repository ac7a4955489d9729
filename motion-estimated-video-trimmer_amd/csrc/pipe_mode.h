// pipe_mode.h — the ONE scan a pipe runs, and what the modes' setters say to each other, as data.  No HIP: pipe.hip
// includes it, and so does a stand-alone program of the CPU tests (tests/test_pipe_mode_host.py) that prints the tables.
//
// A pipe runs exactly one of six scans.  The keep mask (mtgpu_pipe_set_keep) is orthogonal: every mode runs under it.
// The modes exclude each other — a setter turns its mode on only while the pipe runs the plain scan or that same mode —
// so at most one is ever on, and the order in which a setter would look at "the others" is unobservable: there is one
// other at the most, and PIPE_REFUSALS[has][wanted] is the whole answer.
#pragma once

#include <cstdint>

#include "../../include/mtgpu.h"

enum pipe_mode {
  PIPE_PLAIN = 0,   // ctx_launch_scan, or ctx_launch_zones under a keep mask
  PIPE_BLOBS,       // mtgpu_pipe_set_blobs      min_blob, report
  PIPE_GMC,         // mtgpu_pipe_set_gmc        max_shift, min_share_q8, report
  PIPE_GMC_BLOBS,   // mtgpu_pipe_set_gmc_blobs  min_blob, max_shift, min_share_q8, report
  PIPE_DIR,         // mtgpu_pipe_set_dir        allow, report
  PIPE_PLANE,       // mtgpu_pipe_set_plane      report (the plane's bytes live in the pipe: d_plane / h_plane)
  PIPE_MODES
};

// The settings of the mode that is on; a field its mode does not use is 0.  All 0 with PIPE_PLAIN.
struct pipe_settings {
  int32_t min_blob, max_shift, min_share_q8, allow;
  int report;       // MT_PIPE_REPORT_*: which count the batch's ONE count array receives
};

// "a batch of this pipe is being filled / in flight: submit / collect it (or release it) before changing the ..."
// The plain scan has no setter: its slot holds the words of the keep mask's, the one setting next to the mode.
static const char *const PIPE_BUSY_FMT = "a batch of this pipe is %s: submit / collect it (or release it) before changing the %s";
static const char *const PIPE_BUSY_WORDS[PIPE_MODES] = {
    "keep mask", "blob setting", "compensation setting", "compensated blob setting", "direction setting", "direction plane"};

// Report codes: every code but MT_PIPE_REPORT_CENTRES needs a pipe with MT_LAYOUT_CENTRES —
// "<name> needs a pipe with MT_LAYOUT_CENTRES: the <travels> travels in its count array".
struct pipe_report_code { int code; const char *name, *travels; };
static const pipe_report_code PIPE_REPORT_CODES[] = {
    {MT_PIPE_REPORT_CENTRES, "MT_PIPE_REPORT_CENTRES", nullptr},
    {MT_PIPE_REPORT_LARGEST, "MT_PIPE_REPORT_LARGEST", "largest blob"},
    {MT_PIPE_REPORT_VECTOR, "MT_PIPE_REPORT_VECTOR", "applied vector"},
    {MT_PIPE_REPORT_SECTORS, "MT_PIPE_REPORT_SECTORS", "sector word"}};
static const char *const PIPE_REPORT_FMT = "report is %d: want %s";
static const char *const PIPE_REPORT_CENTRES_FMT = "%s needs a pipe with MT_LAYOUT_CENTRES: the %s travels in its count array";
// per mode: the codes its setter accepts (bit `code`), and how the refusal of any other names them
struct pipe_report_rung { unsigned accepts; const char *want; };
static const pipe_report_rung PIPE_REPORT_RUNGS[PIPE_MODES] = {
    {0, nullptr},
    {1u << MT_PIPE_REPORT_CENTRES | 1u << MT_PIPE_REPORT_LARGEST, "MT_PIPE_REPORT_CENTRES or MT_PIPE_REPORT_LARGEST"},
    {1u << MT_PIPE_REPORT_CENTRES | 1u << MT_PIPE_REPORT_VECTOR, "MT_PIPE_REPORT_CENTRES or MT_PIPE_REPORT_VECTOR"},
    {1u << MT_PIPE_REPORT_CENTRES | 1u << MT_PIPE_REPORT_LARGEST | 1u << MT_PIPE_REPORT_VECTOR,
     "MT_PIPE_REPORT_CENTRES, MT_PIPE_REPORT_LARGEST or MT_PIPE_REPORT_VECTOR"},
    {1u << MT_PIPE_REPORT_CENTRES | 1u << MT_PIPE_REPORT_SECTORS, "MT_PIPE_REPORT_CENTRES or MT_PIPE_REPORT_SECTORS"},
    {1u << MT_PIPE_REPORT_CENTRES | 1u << MT_PIPE_REPORT_SECTORS, "MT_PIPE_REPORT_CENTRES or MT_PIPE_REPORT_SECTORS"}};

// The entry of PIPE_REPORT_CODES a mode's setter accepts for `report`, or nullptr.
inline const pipe_report_code *pipe_report_accepted(pipe_mode x, int report) {
  if (report < 0 || report >= 32 || !(PIPE_REPORT_RUNGS[x].accepts >> report & 1u)) return nullptr;
  for (const pipe_report_code &r : PIPE_REPORT_CODES)
    if (r.code == report) return &r;
  return nullptr;
}

// PIPE_REFUSALS[has][wanted]: the pipe runs `has`, a setter wants to turn `wanted` on.  Row and column PIPE_PLAIN and
// the diagonal are empty: nothing refuses the plain scan, and a mode's setter may change its own settings.
struct pipe_refusal { int code; const char *text; };
static const pipe_refusal PIPE_REFUSALS[PIPE_MODES][PIPE_MODES] = {
    /* has plain */ {},
    /* has blobs */
    {{},
     {},
     {MT_ERR_UNSUPPORTED, "this pipe runs the blob scan (mtgpu_pipe_set_blobs): blobs and compensation are not together yet"},
     {MT_ERR_INVALID, "this pipe runs the blob scan (mtgpu_pipe_set_blobs): turn it off first (mtgpu_pipe_set_blobs(pipe, 0, 0)), then call mtgpu_pipe_set_gmc_blobs"},
     {MT_ERR_UNSUPPORTED, "this pipe runs the blob scan (mtgpu_pipe_set_blobs): blobs and direction are not together yet"},
     {MT_ERR_UNSUPPORTED, "this pipe runs the blob scan (mtgpu_pipe_set_blobs): blobs and direction are not together yet"}},
    /* has gmc */
    {{},
     {MT_ERR_UNSUPPORTED, "this pipe runs the compensated scan (mtgpu_pipe_set_gmc): blobs and compensation are not together yet"},
     {},
     {MT_ERR_INVALID, "this pipe runs the compensated scan (mtgpu_pipe_set_gmc): turn it off first (mtgpu_pipe_set_gmc(pipe, 0, 0, 0, 0)), then call mtgpu_pipe_set_gmc_blobs"},
     {MT_ERR_UNSUPPORTED, "this pipe runs the compensated scan (mtgpu_pipe_set_gmc): compensation and direction are not together yet"},
     {MT_ERR_UNSUPPORTED, "this pipe runs the compensated scan (mtgpu_pipe_set_gmc): compensation and direction are not together yet"}},
    /* has gmc_blobs */
    {{},
     {MT_ERR_INVALID, "this pipe runs the compensated blob scan (mtgpu_pipe_set_gmc_blobs): turn it off first, or change min_blob_cells through mtgpu_pipe_set_gmc_blobs"},
     {MT_ERR_INVALID, "this pipe runs the compensated blob scan (mtgpu_pipe_set_gmc_blobs): turn it off first, or change the compensation through mtgpu_pipe_set_gmc_blobs"},
     {},
     {MT_ERR_UNSUPPORTED, "this pipe runs the compensated blob scan (mtgpu_pipe_set_gmc_blobs): the compensated blob scan and direction are not together yet"},
     {MT_ERR_UNSUPPORTED, "this pipe runs the compensated blob scan (mtgpu_pipe_set_gmc_blobs): the compensated blob scan and direction are not together yet"}},
    /* has dir */
    {{},
     {MT_ERR_UNSUPPORTED, "this pipe runs the direction scan (mtgpu_pipe_set_dir): blobs and direction are not together yet"},
     {MT_ERR_UNSUPPORTED, "this pipe runs the direction scan (mtgpu_pipe_set_dir): compensation and direction are not together yet"},
     {MT_ERR_UNSUPPORTED, "this pipe runs the direction scan (mtgpu_pipe_set_dir): the compensated blob scan and direction are not together yet"},
     {},
     {MT_ERR_INVALID, "this pipe runs the direction scan (mtgpu_pipe_set_dir): a plane and the allow byte are one rule at two granularities; turn the byte off first (mtgpu_pipe_set_dir(pipe, 0, 0, 0))"}},
    /* has plane */
    {{},
     {MT_ERR_UNSUPPORTED, "this pipe runs the plane scan (mtgpu_pipe_set_plane): blobs and direction are not together yet"},
     {MT_ERR_UNSUPPORTED, "this pipe runs the plane scan (mtgpu_pipe_set_plane): compensation and direction are not together yet"},
     {MT_ERR_UNSUPPORTED, "this pipe runs the plane scan (mtgpu_pipe_set_plane): the compensated blob scan and direction are not together yet"},
     {MT_ERR_INVALID, "this pipe runs the plane scan (mtgpu_pipe_set_plane): a plane and the allow byte are one rule at two granularities; turn the plane off first (mtgpu_pipe_set_plane(pipe, NULL, 0))"},
     {}}};
