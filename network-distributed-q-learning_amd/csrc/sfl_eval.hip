// Policy-bank evaluation on the device (include/sfl.h sfl_bank_eval): k_eval_fold reduces the per-env
// outputs of the episode launch into one cell of 15 int64 words per policy, behind that launch on the handle's stream,
// in a translation unit of its own (it shares nothing with the wave kernels).
//
// One lane per env: the lanes of a wavefront read consecutive envs of the [E] and [T][E] arrays (coalesced), each lane
// classifies its env's T trains.  With few policies most lanes of a wavefront land in the same cell, so a wavefront
// reduces before it touches memory, as k_curve_fold does (sfl_curve.hip): it takes the first pending lane's policy,
// ballots the lanes on it, reduces their words across the wavefront (sum, min or max by word; the other lanes
// contribute the identity) and lets one lane issue that cell's 64-bit integer atomics.  A lane alone on its policy
// (many policies, env_policy = e % P) skips the reduction: such lanes issue their own atomics together after the loop.
// Every word is an integer, so the cells do not depend on the order the atomics arrive in.
// Only vector loads and stores and global atomics.
#include <hip/hip_runtime.h>

#include "sfl_eval.h"

namespace {

using sfl::EV_WORDS;
using sfl::EvalArgs;

constexpr int EV_BLOCK = 256;
enum { OP_SUM = 0, OP_MIN = 1, OP_MAX = 2 };
__host__ __device__ constexpr int op_of(int k) {
  return (k == sfl::EV_ARR_MIN || k == sfl::EV_REW_MIN) ? OP_MIN : (k == sfl::EV_ARR_MAX || k == sfl::EV_REW_MAX) ? OP_MAX : OP_SUM;
}

template <int OP>
__device__ __forceinline__ int64_t wave_reduce(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t w = (int64_t)__shfl_xor((long long)v, o);
    v = OP == OP_SUM ? v + w : OP == OP_MIN ? (w < v ? w : v) : (w > v ? w : v);
  }
  return v;
}

// one cell's words into memory (every contribution holds at least one episode): the sums that are not zero, min, max
__device__ __forceinline__ void emit(int64_t* c, const int64_t (&v)[EV_WORDS]) {
#pragma unroll
  for (int k = 0; k < EV_WORDS; ++k) {
    if (op_of(k) == OP_SUM) {
      if (v[k] != 0) __hip_atomic_fetch_add(c + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (op_of(k) == OP_MIN) {
      __hip_atomic_fetch_min(c + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      __hip_atomic_fetch_max(c + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ void __launch_bounds__(EV_BLOCK) k_eval_fold(EvalArgs a) {
  const uint32_t e = blockIdx.x * EV_BLOCK + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  const bool in = e < a.E;
  int64_t v[EV_WORDS];
  sfl::eval_cell_clear(v);  // the identity of every word's reduction
  uint32_t key = 0xFFFFFFFFu;
  if (in) {
    key = a.policy[e];  // (< n_policies: sfl_bank_eval checked it)
    sfl::eval_env_cell(a, e, v);
  }
  uint64_t pending = __ballot(in);
  bool solo = false;
  while (pending) {  // (wave-uniform)
    const int leader = __ffsll((unsigned long long)pending) - 1;
    const uint32_t k0 = (uint32_t)__shfl((int)key, leader);
    const bool mine = in && key == k0;
    const uint64_t match = __ballot(mine);
    if (__popcll(match) == 1) {
      solo = solo || mine;
    } else {
      int64_t ident[EV_WORDS], r[EV_WORDS];
      sfl::eval_cell_clear(ident);
#pragma unroll
      for (int k = 0; k < EV_WORDS; ++k) {
        const int64_t x = mine ? v[k] : ident[k];
        r[k] = op_of(k) == OP_SUM ? wave_reduce<OP_SUM>(x) : op_of(k) == OP_MIN ? wave_reduce<OP_MIN>(x) : wave_reduce<OP_MAX>(x);
      }
      if (lane == leader) emit(a.cells + (size_t)k0 * EV_WORDS, r);
    }
    pending &= ~match;
  }
  if (solo) emit(a.cells + (size_t)key * EV_WORDS, v);
}

// the cells emptied: one lane per word
__global__ void __launch_bounds__(EV_BLOCK) k_eval_reset(int64_t* cells, uint32_t n_policies) {
  const size_t i = (size_t)blockIdx.x * EV_BLOCK + threadIdx.x;
  if (i >= (size_t)n_policies * EV_WORDS) return;
  const int k = (int)(i % EV_WORDS);
  cells[i] = op_of(k) == OP_MIN ? INT64_MAX : op_of(k) == OP_MAX ? INT64_MIN : 0;
}

}  // namespace

namespace sfl {

int eval_launch(const EvalArgs& a, void* stream, const char** what, int* code) {
  hipStream_t st = (hipStream_t)stream;
  const unsigned rb = (unsigned)(((size_t)a.n_policies * EV_WORDS + EV_BLOCK - 1) / EV_BLOCK);
  k_eval_reset<<<rb, EV_BLOCK, 0, st>>>(a.cells, a.n_policies);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) {
    *what = "k_eval_reset";
    *code = (int)rc;
    return -1;
  }
  k_eval_fold<<<(a.E + EV_BLOCK - 1) / EV_BLOCK, EV_BLOCK, 0, st>>>(a);
  rc = hipGetLastError();
  if (rc != hipSuccess) {
    *what = "k_eval_fold";
    *code = (int)rc;
    return -1;
  }
  return 0;
}

}  // namespace sfl
