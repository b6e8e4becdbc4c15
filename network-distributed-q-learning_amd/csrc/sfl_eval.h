// Policy-bank evaluation (include/sfl.h sfl_bank_*): the per-policy cell, the work description both
// backends take, and the host build's plain loop.  The rule is stated once, in include/sfl.h; eval_fold_host below, the
// kernel of sfl_eval.hip and the tests' numpy restatement (tests/_evalbank.py) are three implementations of it that
// agree exactly: every word is an integer, so the cells do not depend on the order the envs are folded in.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sfl.h"
#include "sfl_cells.h"
#include "sfl_launch.h"

namespace sfl {

// a cell as 15 int64 words, in the order of sfl_eval_cell
enum {
  EV_EPISODES = 0, EV_EARLY, EV_LATE, EV_NOT_ARR, EV_ARR_MIN, EV_ARR_MAX, EV_ALL_ARR, EV_REW_SUM, EV_REW_MIN, EV_REW_MAX,
  EV_DEC_SUM, EV_TICK_SUM, EV_MF_SUM, EV_DELAY_ARR, EV_TRUNC, EV_WORDS
};
static_assert(sizeof(sfl_eval_cell) == EV_WORDS * 8, "sfl_eval_cell is 15 int64 words");

struct EvalArgs {
  uint32_t E, n_policies;
  int32_t T;
  const uint32_t* policy;      // [E] the table each env followed
  const double* cum;           // the episode launch's per-env outputs: [E] ...
  const int32_t* arrived;
  const int32_t* mf;
  const int32_t* dec;
  const int32_t* ticks;
  const int32_t* trunc;
  const int32_t* delays;       // ... and [T][E]
  const uint8_t* at_dest;      // [T][E]
  int64_t* cells;              // [n_policies][EV_WORDS]
};

// the per-policy cell's layout (sfl_cells.h): each word's reduction and what an empty cell holds there
struct EvalCell {
  static constexpr int N = EV_WORDS, COUNT = EV_EPISODES;  // (a contribution is one episode: COUNT is 1 in each)
  SFL_CELL_FN static constexpr int op(int k) {
    return (k == EV_ARR_MIN || k == EV_REW_MIN) ? OP_MIN : (k == EV_ARR_MAX || k == EV_REW_MAX) ? OP_MAX : OP_SUM;
  }
  SFL_CELL_FN static constexpr int64_t identity(int k) { return cell_op_identity(op(k)); }
};

// env e's episode as a cell of one episode.  The per-train rule is plot.ipynb cell 15's (scripts/eval_table.py
// classify), by train handle: arrived with delay <= 0 is early, arrived with delay > 0 late, anything else not
// arrived -- whose delay is not counted
SFL_CELL_FN void eval_env_cell(const EvalArgs& a, uint32_t e, int64_t* v) {
  const size_t E = a.E;
  cell_clear<EvalCell>(v);
  int64_t early = 0, late = 0, dsum = 0;
  for (int32_t h = 0; h < a.T; ++h) {
    const int64_t d = a.delays[(size_t)h * E + e];
    const bool at = a.at_dest[(size_t)h * E + e] != 0;
    early += (at && d <= 0) ? 1 : 0;
    late += (at && d > 0) ? 1 : 0;
    dsum += at ? d : 0;
  }
  const int64_t arrived = a.arrived[e], reward = (int64_t)a.cum[e];
  v[EV_EPISODES] = 1;
  v[EV_EARLY] = early;
  v[EV_LATE] = late;
  v[EV_NOT_ARR] = (int64_t)a.T - early - late;
  v[EV_ARR_MIN] = v[EV_ARR_MAX] = arrived;
  v[EV_ALL_ARR] = arrived == a.T ? 1 : 0;
  v[EV_REW_SUM] = v[EV_REW_MIN] = v[EV_REW_MAX] = reward;
  v[EV_DEC_SUM] = a.dec[e];
  v[EV_TICK_SUM] = a.ticks[e];
  v[EV_MF_SUM] = a.mf[e];
  v[EV_DELAY_ARR] = dsum;
  v[EV_TRUNC] = a.trunc[e] ? 1 : 0;
}

// The host build: the cells emptied, then in env order, one contribution at a time, no wave logic ("device" memory is
// host memory here).
inline void eval_fold_host(const EvalArgs& a) {
  cells_reset_host<EvalCell>(a.cells, a.n_policies);
  for (uint32_t e = 0; e < a.E; ++e) {
    int64_t v[EV_WORDS];
    eval_env_cell(a, e, v);
    cell_merge<EvalCell>(a.cells + (size_t)a.policy[e] * EV_WORDS, v);
  }
}

// sfl_eval.hip: queues the kernel that empties the cells and k_eval_fold behind it on `stream` (a hipStream_t); the
// failing launch, if any (sfl_launch.h)
LaunchErr eval_launch(const EvalArgs& a, void* stream);

}  // namespace sfl
