// Policy-bank evaluation on the device (include/sfl.h sfl_bank_eval): k_eval_fold reduces the per-env
// outputs of the episode launch into one cell of 15 int64 words per policy, behind that launch on the handle's stream,
// in a translation unit of its own (it shares nothing with the wave kernels).
//
// One lane per env: the lanes of a wavefront read consecutive envs of the [E] and [T][E] arrays (coalesced), each lane
// classifies its env's T trains (eval_env_cell).  The contributions then go through one step of the keyed-cell fold of
// sfl_cells.h (wave_fold), keyed by policy: with few policies most lanes of a wavefront land in the same
// cell and are reduced before they touch memory; with many (env_policy = e % P) a lane is alone on its policy and
// issues its own atomics.
// Only vector loads and stores and global atomics.
#include <hip/hip_runtime.h>

#include "sfl_eval.h"

namespace {

using sfl::EV_WORDS;
using sfl::EvalArgs;

constexpr int EV_BLOCK = 256;

__global__ void __launch_bounds__(EV_BLOCK) k_eval_fold(EvalArgs a) {
  const uint32_t e = blockIdx.x * EV_BLOCK + threadIdx.x;
  const bool in = e < a.E;
  int64_t v[EV_WORDS];
  sfl::cell_clear<sfl::EvalCell>(v);  // the identity of every word's reduction
  uint32_t key = 0xFFFFFFFFu;
  if (in) {
    key = a.policy[e];  // (< n_policies: sfl_bank_eval checked it)
    sfl::eval_env_cell(a, e, v);
  }
  sfl::wave_fold<sfl::EvalCell>(a.cells, threadIdx.x & 63u, in, __ballot(in), key, v);
}

// the cells emptied: one lane per word
__global__ void __launch_bounds__(EV_BLOCK) k_eval_reset(int64_t* cells, uint32_t n_policies) {
  sfl::cells_reset<sfl::EvalCell>(cells, (size_t)blockIdx.x * EV_BLOCK + threadIdx.x, (size_t)n_policies * EV_WORDS);
}

}  // namespace

namespace sfl {

LaunchErr eval_launch(const EvalArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const unsigned rb = (unsigned)(((size_t)a.n_policies * EV_WORDS + EV_BLOCK - 1) / EV_BLOCK);
  k_eval_reset<<<rb, EV_BLOCK, 0, st>>>(a.cells, a.n_policies);
  if (LaunchErr e = launch_err("k_eval_reset")) return e;
  k_eval_fold<<<(a.E + EV_BLOCK - 1) / EV_BLOCK, EV_BLOCK, 0, st>>>(a);
  return launch_err("k_eval_fold");
}

}  // namespace sfl
