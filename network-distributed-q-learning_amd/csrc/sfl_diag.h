// Policy-bank evaluation, the non-arrival diagnosis (include/sfl.h sfl_bank_diag*): the per-policy cell, the
// work description both backends take, the per-train rule as functions both builds share, and the host build's plain
// loops.  The rule is stated once, in include/sfl.h; diag_classify_host / diag_fold_host below, the kernels of
// sfl_diag.hip and the tests' restatement on the Python oracle (tests/_diag.py) are three implementations of it that
// agree exactly: every word is an integer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sfl.h"
#include "sfl_cells.h"
#include "sfl_launch.h"

namespace sfl {

// a cell as 12 int64 words, in the order of sfl_diag_cell
enum {
  DG_EPISODES = 0, DG_TRUNC, DG_NEVER, DG_MOVING, DG_STOP, DG_QUEUE, DG_CYCLE, DG_CYCLES, DG_JAMMED, DG_STALL_MF,
  DG_SF_SUM, DG_SF_MAX, DG_WORDS
};
static_assert(sizeof(sfl_diag_cell) == DG_WORDS * 8, "sfl_diag_cell is 12 int64 words");
static_assert(DG_TRUNC == SFL_DIAG_TRUNCATED && DG_CYCLE == SFL_DIAG_DEADLOCK_CYCLE, "class c is counted in word c");

// the train-state field of a tr_bits word (sfl_core.h tb_state / tb_dir, S_MALF, S_DONE), restated: this header is
// compiled without sfl_core.h
enum : uint32_t { DG_S_MALF = 5, DG_S_DONE = 6 };
enum { DG_MAX_T = 128 };  // trains per env (sfl_create refuses more)

struct DiagArgs {
  uint32_t E, n_policies, HW;
  int32_t T, stall;
  int32_t wave;                // the handle's state layout class: 1 tr_pos / tr_bits are [E][T], 0 [T][E]
  const uint32_t* policy;      // [E] the table each env followed
  const int32_t* ticks;        // [E] the episode launch's outputs ...
  const int32_t* trunc;        // [E]
  const int32_t* last_move;    // [T][E] ... and L, the tick of each train's last move
  const int32_t* tr_pos;       // the envs' end state (SflState)
  const uint32_t* tr_bits;
  const uint32_t* move_tab;    // [HW][4 dir][4 action & 3] (SflMap)
  uint8_t* cls;                // [T][E]
  int16_t* blocker;            // [T][E]
  int32_t* stalled_for;        // [T][E]
  int32_t* env_aux;            // [2][E]: the env's distinct cycles; its stalled trains in state MALFUNCTION
  uint32_t* hot;               // [n_policies][HW]
  int64_t* cells;              // [n_policies][DG_WORDS]
};

struct DiagCell {
  static constexpr int N = DG_WORDS, COUNT = DG_EPISODES;
  SFL_CELL_FN static constexpr int op(int k) { return k == DG_SF_MAX ? OP_MAX : OP_SUM; }
  SFL_CELL_FN static constexpr int64_t identity(int k) { return cell_op_identity(op(k)); }
};

// ---- the rule, per train ------------------------------------------------------------------------------------------------
SFL_CELL_FN size_t diag_state_ix(const DiagArgs& a, uint32_t e, int h) {
  return a.wave ? (size_t)e * (uint32_t)a.T + (uint32_t)h : (size_t)h * a.E + e;
}
SFL_CELL_FN int32_t diag_stalled_for(int32_t n, int32_t L, int32_t pos) { return pos >= 0 ? n - L : -1; }
SFL_CELL_FN bool diag_is_stalled(int32_t sf, int32_t n, int32_t stall) { return sf >= 0 && sf >= (stall < n ? stall : n) - 1; }
// the cells MOVE_FORWARD, MOVE_LEFT, MOVE_RIGHT lead to from (pos, dir), in that order; -1: the action is not valid
SFL_CELL_FN void diag_candidates(const DiagArgs& a, int32_t pos, uint32_t dir, int32_t (&c)[3]) {
  c[0] = c[1] = c[2] = -1;
  if (pos < 0 || (uint32_t)pos >= a.HW) return;
  const uint32_t* row = a.move_tab + ((size_t)pos * 4u + (dir & 3u)) * 4u;
  const uint32_t w[3] = {row[2], row[1], row[3]};  // (A_FWD = 2, A_LEFT = 1, A_RIGHT = 3)
  for (int i = 0; i < 3; ++i)
    if (((w[i] >> 22) & 3u) == 3u) c[i] = (int32_t)(w[i] & 0xFFFFFu) - 1;  // transition valid and new cell valid
}
SFL_CELL_FN uint8_t diag_class(uint32_t state, bool trunc, int32_t pos, bool stalled, int32_t blocker, bool on_cycle) {
  if (state == DG_S_DONE) return SFL_DIAG_ARRIVED;
  if (trunc) return SFL_DIAG_TRUNCATED;
  if (pos < 0) return SFL_DIAG_NEVER_DEPARTED;
  if (!stalled) return SFL_DIAG_MOVING_LATE;
  if (blocker < 0) return SFL_DIAG_STOP_LOOP;
  return on_cycle ? SFL_DIAG_DEADLOCK_CYCLE : SFL_DIAG_DEADLOCK_QUEUE;
}

// env e's diagnosis as a cell of one episode, from what the classify pass wrote
SFL_CELL_FN void diag_env_cell(const DiagArgs& a, uint32_t e, int64_t* v) {
  const size_t E = a.E;
  cell_clear<DiagCell>(v);
  const int32_t n = a.ticks[e];
  int64_t by_class[7] = {0, 0, 0, 0, 0, 0, 0}, sf_sum = 0, sf_max = INT64_MIN;
  for (int32_t h = 0; h < a.T; ++h) {
    const uint32_t c = a.cls[(size_t)h * E + e];
    const int32_t sf = a.stalled_for[(size_t)h * E + e];
    for (uint32_t k = 0; k < 7; ++k) by_class[k] += c == k ? 1 : 0;  // (no dynamic index: registers on the device)
    if (diag_is_stalled(sf, n, a.stall)) {
      sf_sum += sf;
      sf_max = sf > sf_max ? sf : sf_max;
    }
  }
  v[DG_EPISODES] = 1;
  for (int k = 1; k < 7; ++k) v[k] = by_class[k];
  v[DG_CYCLES] = a.env_aux[e];
  v[DG_JAMMED] = by_class[5] + by_class[6] > 0 ? 1 : 0;
  v[DG_STALL_MF] = a.env_aux[E + e];
  v[DG_SF_SUM] = sf_sum;
  v[DG_SF_MAX] = sf_max;
}

// ---- the host build: plain loops ("device" memory is host memory here) ----------------------------------------------------
inline void diag_classify_host(const DiagArgs& a) {
  const size_t E = a.E;
  const int T = a.T;
  for (size_t i = 0; i < (size_t)a.n_policies * a.HW; ++i) a.hot[i] = 0;
  for (uint32_t e = 0; e < a.E; ++e) {
    const int32_t n = a.ticks[e];
    int32_t pos[DG_MAX_T], sf[DG_MAX_T], blk[DG_MAX_T];
    bool stalled[DG_MAX_T];
    uint32_t bits[DG_MAX_T];
    for (int h = 0; h < T; ++h) {
      pos[h] = a.tr_pos[diag_state_ix(a, e, h)];
      bits[h] = a.tr_bits[diag_state_ix(a, e, h)];
      sf[h] = diag_stalled_for(n, a.last_move[(size_t)h * E + e], pos[h]);
      stalled[h] = diag_is_stalled(sf[h], n, a.stall);
    }
    for (int h = 0; h < T; ++h) {
      blk[h] = -1;
      if (!stalled[h]) continue;
      int32_t c[3];
      diag_candidates(a, pos[h], bits[h] & 3u, c);
      for (int i = 0; i < 3 && blk[h] < 0; ++i) {
        if (c[i] < 0) continue;
        int occ = -1;
        for (int j = 0; j < T; ++j)
          if (pos[j] == c[i]) occ = j;
        if (occ >= 0 && stalled[occ]) blk[h] = occ;
      }
    }
    int32_t cycles = 0, stall_mf = 0;
    for (int h = 0; h < T; ++h) {
      int x = blk[h], lo = h;
      for (int s = 0; s < T && x >= 0 && x != h; ++s) {
        lo = x < lo ? x : lo;
        x = blk[x];
      }
      const bool on_cycle = stalled[h] && x == h;
      const uint32_t state = (bits[h] >> 2) & 7u;
      const uint8_t c = diag_class(state, a.trunc[e] != 0, pos[h], stalled[h], blk[h], on_cycle);
      a.cls[(size_t)h * E + e] = c;
      a.blocker[(size_t)h * E + e] = (int16_t)blk[h];
      a.stalled_for[(size_t)h * E + e] = sf[h];
      cycles += (c == SFL_DIAG_DEADLOCK_CYCLE && lo == h) ? 1 : 0;
      stall_mf += (stalled[h] && state == DG_S_MALF) ? 1 : 0;
      if (c >= SFL_DIAG_STOP_LOOP && (uint32_t)pos[h] < a.HW) a.hot[(size_t)a.policy[e] * a.HW + (uint32_t)pos[h]] += 1;
    }
    a.env_aux[e] = cycles;
    a.env_aux[E + e] = stall_mf;
  }
}

inline void diag_fold_host(const DiagArgs& a) {
  cells_reset_host<DiagCell>(a.cells, a.n_policies);
  for (uint32_t e = 0; e < a.E; ++e) {
    int64_t v[DG_WORDS];
    diag_env_cell(a, e, v);
    cell_merge<DiagCell>(a.cells + (size_t)a.policy[e] * DG_WORDS, v);
  }
}

// sfl_diag.hip: queues the kernel that empties the cells and `hot`, k_diag_classify and k_diag_fold on `stream` (a
// hipStream_t); the failing launch, if any (sfl_launch.h)
LaunchErr diag_launch(const DiagArgs& a, void* stream);

}  // namespace sfl
