// make_plan (mad_icp_amd/csrc/common/launch_plan.h) over a list of launches, for tests/test_registration_history_inputs.py:
// stdin holds one launch per line — max_L K batch iters trace — and every line is answered by one line
//   grid partial_doubles tie
// under default options and n_cus = 256.  `tie` is every member of Plan::tie() joined with '/': two launches share a captured
// graph iff their ties (and their Job arrays) are equal.  partial_doubles restates partial_doubles_of (madicp_capi.hip), which
// the Python side pins to the source by its text; the first line printed is the floor of ensure_partials, 2 * 288 * kAcc * 8.
#include <cstdio>

#include "launch_plan.h"

using namespace madicp;

static size_t align_up(size_t v) { return (v + 255) / 256 * 256; }
static size_t partial_doubles_of(int grid, int n_scans) {
  const size_t prows = (size_t)join_rows(grid);
  return align_up(((size_t)2 * n_scans * prows * kAcc + (size_t)2 * n_scans * grid + kAcc) * sizeof(double)) / sizeof(double);
}

int main() {
  std::printf("%zu\n", (size_t)2 * 288 * kAcc * 8);
  const Options opt;
  PlanEnv env;
  env.n_cus = 256;
  int max_L, K, batch, iters, trace;
  while (std::scanf("%d %d %d %d %d", &max_L, &K, &batch, &iters, &trace) == 5) {
    const Plan p = make_plan(opt, env, max_L, K, batch, iters, trace != 0, max_L <= kP2pFlagLeaves);
    std::printf("%d %zu %d/%d/%d/%d/%d/%d/%d/%d/%d/%d/%d/%d\n", p.grid, partial_doubles_of(p.grid, p.batch), p.batch, p.iters, p.K, p.trace,
                p.grid, p.qpt, p.lds, p.rpt, p.queue, (int)p.route, (int)p.flags_in_box, (int)p.interleave);
  }
  return 0;
}
