// Step-mode learning curves (include/sfl.h sfl_curve_*): the cell layouts (sfl_cells.h), the work description both
// backends take, the one function that builds an episode's (a round's) contribution, and the host build's plain loops.
// The rule is stated once, in include/sfl.h and DESIGN.md §17; curve_fold_host below, the kernel of sfl_curve.hip and
// the test model (tests/_curve.py) are three implementations of it that agree exactly.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sfl.h"
#include "sfl_cells.h"
#include "sfl_launch.h"

namespace sfl {

// a cell as 16 int64 words, in the order of sfl_curve_cell
enum {
  CV_COUNT = 0, CV_LOST, CV_ARR_SUM, CV_ARR_MIN, CV_ARR_MAX, CV_ALL_ARR, CV_REW_SUM, CV_REW_MIN, CV_REW_MAX,
  CV_DEC_SUM, CV_TICK_SUM, CV_MF_SUM, CV_DELAY_SUM, CV_TRUNC, CV_EP_FIRST, CV_EP_LAST, CV_WORDS
};
static_assert(sizeof(sfl_curve_cell) == CV_WORDS * 8, "sfl_curve_cell is 16 int64 words");

struct CurveArgs {
  uint32_t E, n_series;
  int32_t T, n_bins, bin_episodes, ring_cap;
  int64_t max_steps;            // an episode is truncated when its decisions exceed it
  const int32_t* ep_t;          // [E] the envs' learning-episode indices
  int32_t* mark;                // [E] episodes accounted for so far
  const uint32_t* series;       // [E]
  const double* st_cum;         // the ring: [ring_cap][E] ...
  const int32_t* st_arrived;
  const int32_t* st_mf;
  const int32_t* st_dec;
  const int32_t* st_ticks;
  const int32_t* st_delays;     // ... and [ring_cap][T][E]
  int64_t* cells;               // [n_bins][n_series][CV_WORDS]
};

SFL_CELL_FN size_t curve_cell_of(const CurveArgs& a, int32_t episode, uint32_t series) {
  int32_t bin = episode / a.bin_episodes;
  if (bin > a.n_bins - 1) bin = a.n_bins - 1;
  return (size_t)bin * a.n_series + series;
}

// the curve's layout (sfl_cells.h): each word's reduction and what an empty cell holds there
struct EpisodeCell {
  static constexpr int N = CV_WORDS, COUNT = CV_COUNT;
  SFL_CELL_FN static constexpr int op(int k) {
    return (k == CV_ARR_MIN || k == CV_REW_MIN || k == CV_EP_FIRST) ? OP_MIN
           : (k == CV_ARR_MAX || k == CV_REW_MAX || k == CV_EP_LAST) ? OP_MAX
                                                                     : OP_SUM;
  }
  // (an empty cell's ep_last reads -1 through sfl_curve_read)
  SFL_CELL_FN static constexpr int64_t identity(int k) { return k == CV_EP_LAST ? -1 : cell_op_identity(op(k)); }
};

// episode i of env e (of series `series`) as a cell of one episode in v; returns the cell it belongs to.  An episode
// below `kept` was overwritten in the ring: it counts as lost and nothing else
SFL_CELL_FN void curve_episode_cell(const CurveArgs& a, uint32_t e, uint32_t series, int32_t i, int32_t kept, int64_t* v,
                                    uint32_t& key) {
  const size_t E = a.E;
  key = (uint32_t)curve_cell_of(a, i, series);
  cell_clear<EpisodeCell>(v);
  if (i < kept) {
    v[CV_LOST] = 1;
  } else {
    const size_t row = (size_t)(i % a.ring_cap);
    const int64_t arrived = a.st_arrived[row * E + e], reward = (int64_t)a.st_cum[row * E + e];
    const int64_t dec = a.st_dec[row * E + e];
    int64_t delay = 0;
    for (int32_t h = 0; h < a.T; ++h) delay += a.st_delays[(row * (size_t)a.T + h) * E + e];
    v[CV_COUNT] = 1;
    v[CV_ARR_SUM] = v[CV_ARR_MIN] = v[CV_ARR_MAX] = arrived;
    v[CV_ALL_ARR] = arrived == a.T ? 1 : 0;
    v[CV_REW_SUM] = v[CV_REW_MIN] = v[CV_REW_MAX] = reward;
    v[CV_DEC_SUM] = dec;
    v[CV_TICK_SUM] = a.st_ticks[row * E + e];
    v[CV_MF_SUM] = a.st_mf[row * E + e];
    v[CV_DELAY_SUM] = delay;
    v[CV_TRUNC] = dec > a.max_steps ? 1 : 0;
    v[CV_EP_FIRST] = v[CV_EP_LAST] = i;
  }
}

// The host build: the rule as written -- in env order, one contribution at a time, no wave logic ("device" memory is
// host memory here).
inline void curve_reset_host(const CurveArgs& a) { cells_reset_host<EpisodeCell>(a.cells, (size_t)a.n_bins * a.n_series); }

inline void curve_fold_host(const CurveArgs& a) {
  for (uint32_t e = 0; e < a.E; ++e) {
    const int32_t end = a.ep_t[e], b = a.mark[e];
    const int32_t kept = end - a.ring_cap > b ? end - a.ring_cap : b;
    for (int32_t i = b; i < end; ++i) {
      int64_t v[CV_WORDS];
      uint32_t key;
      curve_episode_cell(a, e, a.series[e], i, kept, v, key);
      cell_merge<EpisodeCell>(a.cells + (size_t)key * CV_WORDS, v);
    }
    a.mark[e] = end;
  }
}

// ---- the exploit record (include/sfl.h sfl_curve_exploit): the greedy rounds sfl_step runs ----
// an exploit cell as 11 int64 words, in the order of sfl_curve_xcell
enum {
  XV_COUNT = 0, XV_LOST, XV_ARR_SUM, XV_ARR_MIN, XV_ARR_MAX, XV_ALL_ARR, XV_REW_SUM, XV_REW_MIN, XV_REW_MAX, XV_EP_FIRST,
  XV_EP_LAST, XV_WORDS
};
static_assert(sizeof(sfl_curve_xcell) == XV_WORDS * 8, "sfl_curve_xcell is 11 int64 words");
constexpr uint32_t CVX_DONE = 8u;  // F_EXPLOIT_DONE of the env's flags word (sfl_core.h; sfl_engine.h asserts it)

struct CurveXArgs {
  uint32_t E, n_series;
  int32_t T, n_bins, bin_episodes, ring_cap;
  int32_t f;                    // the frequency the rounds are counted with (the last sfl_curve_exploit with f >= 1)
  int32_t period;               // ring_cap / gcd(ring_cap, f): rounds r and r + period share a ring row
  const int32_t* ep_t;          // [E]
  const uint32_t* eflags;       // [E] the envs' flags words
  int32_t* mark;                // [E] rounds accounted for so far
  const int32_t* limit;         // [E] after sfl_curve_exploit(h, 0): the rounds an env can still complete; else null
  const uint32_t* series;       // [E] (the curve's)
  const double* sx_cum;         // the ring: [ring_cap][E]
  const int32_t* sx_arrived;
  int64_t* cells;               // [n_bins][n_series][XV_WORDS]
};

// the rounds an env at episode index a with flags word `flags` has completed under frequency f
SFL_CELL_FN int32_t curve_rounds_done(int32_t a, uint32_t flags, int32_t f) {
  return a / f + (((flags & CVX_DONE) && (a + 1) % f == 0) ? 1 : 0);
}

// the episode round r precedes (never above the env's episode index, so it fits an int32)
SFL_CELL_FN int32_t curve_round_episode(int32_t r, int32_t f) { return (int32_t)(((int64_t)r + 1) * f - 1); }

SFL_CELL_FN size_t curve_xcell_of(const CurveXArgs& a, int32_t episode, uint32_t series) {
  int32_t bin = episode / a.bin_episodes;
  if (bin > a.n_bins - 1) bin = a.n_bins - 1;
  return (size_t)bin * a.n_series + series;
}

struct ExploitCell {
  static constexpr int N = XV_WORDS, COUNT = XV_COUNT;
  SFL_CELL_FN static constexpr int op(int k) {
    return (k == XV_ARR_MIN || k == XV_REW_MIN || k == XV_EP_FIRST) ? OP_MIN
           : (k == XV_ARR_MAX || k == XV_REW_MAX || k == XV_EP_LAST) ? OP_MAX
                                                                     : OP_SUM;
  }
  // (an empty cell's ep_last reads -1 through sfl_curve_read_exploit)
  SFL_CELL_FN static constexpr int64_t identity(int k) { return k == XV_EP_LAST ? -1 : cell_op_identity(op(k)); }
};

// greedy round r of env e (of series `series`) as a cell of one round in v; returns the cell it belongs to (by the
// episode the round precedes).  A round below `kept` was overwritten in the ring: it counts as lost and nothing else
SFL_CELL_FN void curve_round_cell(const CurveXArgs& a, uint32_t e, uint32_t series, int32_t r, int32_t kept, int64_t* v,
                                  uint32_t& key) {
  const size_t E = a.E;
  const int32_t t = curve_round_episode(r, a.f);
  key = (uint32_t)curve_xcell_of(a, t, series);
  cell_clear<ExploitCell>(v);
  if (r < kept) {
    v[XV_LOST] = 1;
  } else {
    const size_t row = (size_t)(t % a.ring_cap);
    const int64_t arrived = a.sx_arrived[row * E + e], reward = (int64_t)a.sx_cum[row * E + e];
    v[XV_COUNT] = 1;
    v[XV_ARR_SUM] = v[XV_ARR_MIN] = v[XV_ARR_MAX] = arrived;
    v[XV_ALL_ARR] = arrived == a.T ? 1 : 0;
    v[XV_REW_SUM] = v[XV_REW_MIN] = v[XV_REW_MAX] = reward;
    v[XV_EP_FIRST] = v[XV_EP_LAST] = t;
  }
}

// the host build, as curve_fold_host: in env order, one contribution at a time, no wave logic
inline void curve_xreset_host(const CurveXArgs& a) { cells_reset_host<ExploitCell>(a.cells, (size_t)a.n_bins * a.n_series); }

inline void curve_xfold_host(const CurveXArgs& a) {
  for (uint32_t e = 0; e < a.E; ++e) {
    int32_t n = curve_rounds_done(a.ep_t[e], a.eflags[e], a.f);
    if (a.limit && a.limit[e] < n) n = a.limit[e];
    const int32_t b = a.mark[e];
    const int32_t kept = n - a.period > b ? n - a.period : b;
    for (int32_t r = b; r < n; ++r) {
      int64_t v[XV_WORDS];
      uint32_t key;
      curve_round_cell(a, e, a.series[e], r, kept, v, key);
      cell_merge<ExploitCell>(a.cells + (size_t)key * XV_WORDS, v);
    }
    a.mark[e] = n;
  }
}

// sfl_curve.hip: queues one kernel on `stream` (a hipStream_t) -- the fold, or with `reset` the kernel that empties the
// cells; the failing launch, if any (sfl_launch.h)
LaunchErr curve_launch(const CurveArgs& a, bool reset, void* stream);
// the same for the exploit record: k_curve_fold_exploit, or with `reset` the kernel that empties its cells
LaunchErr curve_xlaunch(const CurveXArgs& a, bool reset, void* stream);

}  // namespace sfl
