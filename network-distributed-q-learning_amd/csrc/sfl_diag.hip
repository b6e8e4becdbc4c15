// Policy-bank evaluation, the non-arrival diagnosis on the device (include/sfl.h sfl_bank_diag), in a
// translation unit of its own (it shares nothing with the wave kernels).  Three launches on the handle's stream behind
// the evaluation: k_diag_reset empties the cells and the hotspot counts, k_diag_classify gives every train of every env
// its class, blocker and stalled_for (the rule: include/sfl.h; its per-train functions: sfl_diag.h), k_diag_fold
// reduces the classes into one cell of 12 int64 words per policy through the keyed-cell fold of sfl_cells.h.
//
// k_diag_classify's lane mapping.  An env is a group of GS lanes, GS the power of two with T <= GS (64 at most: above
// that a lane holds two train slots, t and t + 64), so a 256-thread block holds NE = 256 / GS envs.  Every per-train
// array of the pass is [T][E], env-minor.  The block's threads are therefore laid out with the env fastest: thread i is
// train i / NE of the block's env i % NE, so the lanes of a wavefront that hold one train read and write NE (or 64)
// consecutive elements of a row, instead of one element in each of GS rows that lie E elements apart.  The price is that
// a group's lanes are not adjacent in a wavefront (and at GS > 16 not in one wavefront), so the group exchanges its
// final cells, its stalled set and its blockers through the block's LDS, indexed [train][env of the block] -- the
// same order, so every LDS write is conflict-free and every read of another train's word is a broadcast to the lanes
// of the env -- with block barriers between the three steps.  The envs' end state is read in the handle's own layout
// class: [T][E] on the lane-per-env body, [E][T] on the wave kernels, where the block's rows are NE short runs.
// Only vector loads and stores, LDS (with LDS atomics for the env's two counts) and global atomics.
#include <hip/hip_runtime.h>

#include "sfl_diag.h"

namespace {

using sfl::DG_WORDS;
using sfl::DiagArgs;

constexpr int DG_BLOCK = 256;
constexpr int DG_SLOTS = 512;  // train slots of a block: NE * GS * (1 or 2)

__global__ void __launch_bounds__(DG_BLOCK) k_diag_classify(DiagArgs a, int gs_log2) {
  __shared__ int32_t lpos[DG_SLOTS];  // [train][env of the block]: final cell, -1 off the map (or no such train / env)
  __shared__ int32_t lstl[DG_SLOTS];  // 1: stalled
  __shared__ int32_t lblk[DG_SLOTS];  // blocker or -1
  __shared__ int32_t lcnt[2 * DG_BLOCK];  // [2][env of the block]: distinct cycles, stalled trains in MALFUNCTION
  const int ne = DG_BLOCK >> gs_log2;     // envs of a block
  const int gs = 1 << gs_log2;
  const int tpl = (a.T + gs - 1) >> gs_log2;  // train slots per lane: 1, or 2 for T > 64
  const int el = (int)threadIdx.x & (ne - 1), t0 = (int)threadIdx.x / ne;
  const uint32_t e = blockIdx.x * (uint32_t)ne + (uint32_t)el;
  const bool env_ok = e < a.E;
  const size_t E = a.E;
  const int32_t n = env_ok ? a.ticks[e] : 0;
  const bool trunc = env_ok && a.trunc[e] != 0;
  if (t0 == 0) lcnt[el] = lcnt[DG_BLOCK + el] = 0;
  int32_t pos[2], sf[2];
  uint32_t bits[2];
  bool mine[2], stalled[2];
  // step 1: the trains' end state, stalled_for and the stalled set
  for (int k = 0; k < 2; ++k) {
    const int h = t0 + k * gs;
    mine[k] = k < tpl && env_ok && h < a.T;
    pos[k] = -1;
    bits[k] = 0;
    sf[k] = -1;
    stalled[k] = false;
    if (mine[k]) {
      const size_t six = sfl::diag_state_ix(a, e, h);
      pos[k] = a.tr_pos[six];
      bits[k] = a.tr_bits[six];
      sf[k] = sfl::diag_stalled_for(n, a.last_move[(size_t)h * E + e], pos[k]);
      stalled[k] = sfl::diag_is_stalled(sf[k], n, a.stall);
    }
    if (k < tpl) {  // (h < gs * tpl: inside the block's slots; a train or env that does not exist stands nowhere)
      lpos[h * ne + el] = pos[k];
      lstl[h * ne + el] = stalled[k] ? 1 : 0;
    }
  }
  __syncthreads();
  // step 2: the blocker -- the candidate cells against the env's T final cells
  int32_t blk[2];
  for (int k = 0; k < 2; ++k) {
    blk[k] = -1;
    if (k < tpl) {
      int32_t c[3] = {-1, -1, -1}, occ[3] = {-1, -1, -1};
      if (stalled[k]) sfl::diag_candidates(a, pos[k], bits[k] & 3u, c);
      if (stalled[k] && (c[0] >= 0 || c[1] >= 0 || c[2] >= 0)) {
        for (int j = 0; j < a.T; ++j) {
          const int32_t p = lpos[j * ne + el];
          occ[0] = p == c[0] ? j : occ[0];  // (the highest handle on the cell; an off-map train's -1 meets only an
          occ[1] = p == c[1] ? j : occ[1];  // invalid action's -1, which is skipped below)
          occ[2] = p == c[2] ? j : occ[2];
        }
#pragma unroll
        for (int i = 2; i >= 0; --i)  // the first action in order whose cell holds a stalled train
          if (c[i] >= 0 && occ[i] >= 0 && lstl[occ[i] * ne + el] != 0) blk[k] = occ[i];
      }
      lblk[(t0 + k * gs) * ne + el] = blk[k];
    }
  }
  __syncthreads();
  // step 3: the blocker chain, the class, the outputs
  for (int k = 0; k < 2; ++k) {
    const int h = t0 + k * gs;
    if (!mine[k]) continue;
    int x = blk[k], lo = h;
    for (int s = 0; s < a.T && x >= 0 && x != h; ++s) {
      lo = x < lo ? x : lo;
      x = lblk[x * ne + el];
    }
    const bool on_cycle = stalled[k] && x == h;
    const uint32_t state = (bits[k] >> 2) & 7u;
    const uint8_t c = sfl::diag_class(state, trunc, pos[k], stalled[k], blk[k], on_cycle);
    a.cls[(size_t)h * E + e] = c;
    a.blocker[(size_t)h * E + e] = (int16_t)blk[k];
    a.stalled_for[(size_t)h * E + e] = sf[k];
    if (c == SFL_DIAG_DEADLOCK_CYCLE && lo == h) atomicAdd(&lcnt[el], 1);
    if (stalled[k] && state == sfl::DG_S_MALF) atomicAdd(&lcnt[DG_BLOCK + el], 1);
    if (c >= SFL_DIAG_STOP_LOOP && (uint32_t)pos[k] < a.HW)
      atomicAdd(a.hot + (size_t)a.policy[e] * a.HW + (uint32_t)pos[k], 1u);  // (policy < n_policies: sfl_bank_eval checked it)
  }
  __syncthreads();
  if (t0 == 0 && env_ok) {
    a.env_aux[e] = lcnt[el];
    a.env_aux[E + e] = lcnt[DG_BLOCK + el];
  }
}

// one lane per env, as k_eval_fold: the lanes of a wavefront read consecutive envs of the [T][E] arrays
__global__ void __launch_bounds__(DG_BLOCK) k_diag_fold(DiagArgs a) {
  const uint32_t e = blockIdx.x * DG_BLOCK + threadIdx.x;
  const bool in = e < a.E;
  int64_t v[DG_WORDS];
  sfl::cell_clear<sfl::DiagCell>(v);
  uint32_t key = 0xFFFFFFFFu;
  if (in) {
    key = a.policy[e];
    sfl::diag_env_cell(a, e, v);
  }
  sfl::wave_fold<sfl::DiagCell>(a.cells, threadIdx.x & 63u, in, __ballot(in), key, v);
}

// the cells and the hotspot counts emptied: one lane per word
__global__ void __launch_bounds__(DG_BLOCK) k_diag_reset(int64_t* cells, uint32_t n_policies, uint32_t* hot, size_t n_hot) {
  const size_t i = (size_t)blockIdx.x * DG_BLOCK + threadIdx.x;
  sfl::cells_reset<sfl::DiagCell>(cells, i, (size_t)n_policies * DG_WORDS);
  if (i < n_hot) hot[i] = 0u;
}

}  // namespace

namespace sfl {

LaunchErr diag_launch(const DiagArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t n_hot = (size_t)a.n_policies * a.HW, n_words = (size_t)a.n_policies * DG_WORDS;
  const size_t n_reset = n_hot > n_words ? n_hot : n_words;
  k_diag_reset<<<(unsigned)((n_reset + DG_BLOCK - 1) / DG_BLOCK), DG_BLOCK, 0, st>>>(a.cells, a.n_policies, a.hot, n_hot);
  if (LaunchErr e = launch_err("k_diag_reset")) return e;
  int gs_log2 = 0;
  while ((1 << gs_log2) < a.T && gs_log2 < 6) ++gs_log2;
  const uint32_t ne = (uint32_t)DG_BLOCK >> gs_log2;
  k_diag_classify<<<(a.E + ne - 1) / ne, DG_BLOCK, 0, st>>>(a, gs_log2);
  if (LaunchErr e = launch_err("k_diag_classify")) return e;
  k_diag_fold<<<(a.E + DG_BLOCK - 1) / DG_BLOCK, DG_BLOCK, 0, st>>>(a);
  return launch_err("k_diag_fold");
}

}  // namespace sfl
