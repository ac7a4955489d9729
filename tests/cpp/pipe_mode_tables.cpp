// Prints the tables of csrc/pipe_mode.h, one tab-separated line per entry, for tests/test_pipe_mode_host.py.  Stand-alone:
// no HIP, no library.
//   refusal <has> <wanted> <code> <text>
//   busy    <mode> <state> <text>
//   report  <mode> <centres 0/1> <report> <code> <text>      code 0: accepted
#include <cstdio>
#include <initializer_list>

#include "pipe_mode.h"

int main() {
  char text[512];
  for (int has = PIPE_PLAIN + 1; has < PIPE_MODES; ++has)
    for (int wanted = PIPE_PLAIN + 1; wanted < PIPE_MODES; ++wanted)
      if (has != wanted) std::printf("refusal\t%d\t%d\t%d\t%s\n", has, wanted, PIPE_REFUSALS[has][wanted].code, PIPE_REFUSALS[has][wanted].text);
  for (int x = PIPE_PLAIN; x < PIPE_MODES; ++x)
    for (const char *state : {"being filled", "in flight"}) {
      std::snprintf(text, sizeof text, PIPE_BUSY_FMT, state, PIPE_BUSY_WORDS[x]);
      std::printf("busy\t%d\t%s\t%s\n", x, state, text);
    }
  for (int x = PIPE_PLAIN + 1; x < PIPE_MODES; ++x)
    for (int centres = 0; centres < 2; ++centres)
      for (int report = -1; report <= 5; ++report) {
        const pipe_report_code *r = pipe_report_accepted((pipe_mode)x, report);
        int code = 0;
        text[0] = 0;
        if (!r) { code = MT_ERR_INVALID; std::snprintf(text, sizeof text, PIPE_REPORT_FMT, report, PIPE_REPORT_RUNGS[x].want); }
        else if (r->travels && !centres) { code = MT_ERR_INVALID; std::snprintf(text, sizeof text, PIPE_REPORT_CENTRES_FMT, r->name, r->travels); }
        std::printf("report\t%d\t%d\t%d\t%d\t%s\n", x, centres, report, code, text);
      }
  return 0;
}
