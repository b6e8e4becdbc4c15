// Step-mode learning curves on the device (include/sfl.h sfl_curve_*; the rule: DESIGN.md §17).
//
// k_curve_fold reduces the statistics rows a step launch wrote into the handle's ring into the (bin, series) cells, in
// a translation unit of its own (it shares nothing with the wave kernels).  One lane per env: the lanes of a wavefront
// read consecutive envs of the [row][E] ring arrays (the T delay rows [(row * T + h) * E + e] too), each lane walks its
// own finished episodes and the wavefront loops to its longest lane.  Nearly every env of a launch lands in the same
// one or two cells, so a wavefront reduces before it touches memory: per step it takes the first pending lane's cell,
// ballots the lanes on the same cell, reduces their 16 words across the wavefront (sum, min or max by word; lanes on
// another cell contribute the identity) and lets one lane issue that cell's 64-bit integer atomics.  A lane alone on
// its cell (one series per env) skips the reduction: such lanes issue their own atomics together after the loop.
// Every word is an integer, so the cells do not depend on the order the atomics arrive in.
// Only vector loads and stores and global atomics.
#include <hip/hip_runtime.h>

#include "sfl_curve.h"

namespace {

using sfl::CurveArgs;
using sfl::CV_WORDS;

constexpr int CV_BLOCK = 256;

enum { OP_SUM = 0, OP_MIN = 1, OP_MAX = 2 };
__host__ __device__ constexpr int word_op(int k) {
  return (k == sfl::CV_ARR_MIN || k == sfl::CV_REW_MIN || k == sfl::CV_EP_FIRST) ? OP_MIN
         : (k == sfl::CV_ARR_MAX || k == sfl::CV_REW_MAX || k == sfl::CV_EP_LAST) ? OP_MAX
                                                                                  : OP_SUM;
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

// one cell's words into memory: the sums that are not zero; min / max only when an episode was folded
__device__ __forceinline__ void emit(int64_t* c, const int64_t (&v)[CV_WORDS]) {
#pragma unroll
  for (int k = 0; k < CV_WORDS; ++k) {
    if (word_op(k) == OP_SUM) {
      if (v[k] != 0) __hip_atomic_fetch_add(c + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (v[sfl::CV_COUNT] != 0) {
      if (word_op(k) == OP_MIN) __hip_atomic_fetch_min(c + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else __hip_atomic_fetch_max(c + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ void __launch_bounds__(CV_BLOCK) k_curve_fold(CurveArgs a) {
  const uint32_t e = blockIdx.x * CV_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const bool in = e < a.E;
  const size_t E = a.E;
  int32_t b = 0, end = 0;
  uint32_t ser = 0;
  if (in) {
    end = a.ep_t[e];
    b = a.mark[e];
    ser = a.series[e];
  }
  const int32_t kept = end - a.ring_cap > b ? end - a.ring_cap : b;  // the episodes below it were overwritten
  for (int32_t i = b;; ++i) {  // (every lane of a wavefront starts at its own mark: step k is episode mark + k)
    const bool active = in && i < end;
    uint64_t pending = __ballot(active);
    if (!pending) break;
    int64_t v[CV_WORDS];
    sfl::curve_cell_clear(v);  // the identity of every word's reduction
    uint32_t key = 0xFFFFFFFFu;
    if (active) {
      key = (uint32_t)sfl::curve_cell_of(a, i, ser);
      if (i < kept) {
        v[sfl::CV_LOST] = 1;
      } else {
        const size_t row = (size_t)(i % a.ring_cap);
        const int64_t arrived = a.st_arrived[row * E + e], reward = (int64_t)a.st_cum[row * E + e];
        const int64_t dec = a.st_dec[row * E + e];
        int64_t delay = 0;
        for (int32_t h = 0; h < a.T; ++h) delay += a.st_delays[(row * (size_t)a.T + h) * E + e];
        v[sfl::CV_COUNT] = 1;
        v[sfl::CV_ARR_SUM] = v[sfl::CV_ARR_MIN] = v[sfl::CV_ARR_MAX] = arrived;
        v[sfl::CV_ALL_ARR] = arrived == a.T ? 1 : 0;
        v[sfl::CV_REW_SUM] = v[sfl::CV_REW_MIN] = v[sfl::CV_REW_MAX] = reward;
        v[sfl::CV_DEC_SUM] = dec;
        v[sfl::CV_TICK_SUM] = a.st_ticks[row * E + e];
        v[sfl::CV_MF_SUM] = a.st_mf[row * E + e];
        v[sfl::CV_DELAY_SUM] = delay;
        v[sfl::CV_TRUNC] = dec > a.max_steps ? 1 : 0;
        v[sfl::CV_EP_FIRST] = v[sfl::CV_EP_LAST] = i;
      }
    }
    bool solo = false;
    while (pending) {  // the distinct cells among the active lanes (wave-uniform: pending and match are ballots)
      const int leader = __ffsll((unsigned long long)pending) - 1;
      const uint32_t k0 = (uint32_t)__shfl((int)key, leader);
      const bool mine = active && key == k0;
      const uint64_t match = __ballot(mine);
      if (__popcll(match) == 1) {
        solo = solo || mine;
      } else {
        int64_t ident[CV_WORDS], r[CV_WORDS];
        sfl::curve_cell_clear(ident);
#pragma unroll
        for (int k = 0; k < CV_WORDS; ++k) {
          const int64_t x = mine ? v[k] : ident[k];
          r[k] = word_op(k) == OP_SUM ? wave_reduce<OP_SUM>(x) : word_op(k) == OP_MIN ? wave_reduce<OP_MIN>(x) : wave_reduce<OP_MAX>(x);
        }
        if ((int)lane == leader) emit(a.cells + (size_t)k0 * CV_WORDS, r);
      }
      pending &= ~match;
    }
    if (solo) emit(a.cells + (size_t)key * CV_WORDS, v);
  }
  if (in) a.mark[e] = end;
}

// the cells emptied (sfl_curve_begin, sfl_learn_begin): one lane per word
__global__ void __launch_bounds__(CV_BLOCK) k_curve_reset(CurveArgs a) {
  const size_t i = (size_t)blockIdx.x * CV_BLOCK + threadIdx.x;
  if (i >= (size_t)a.n_bins * a.n_series * CV_WORDS) return;
  int64_t ident[CV_WORDS];
  sfl::curve_cell_clear(ident);
  int64_t x = 0;
#pragma unroll
  for (int k = 0; k < CV_WORDS; ++k) x = (int)(i % CV_WORDS) == k ? ident[k] : x;
  a.cells[i] = x;
}

}  // namespace

namespace sfl {

int curve_launch(const CurveArgs& a, bool reset, void* stream_, const char** what, int* code) {
  hipStream_t stream = (hipStream_t)stream_;
  const size_t n = reset ? (size_t)a.n_bins * a.n_series * CV_WORDS : (size_t)a.E;
  const unsigned blocks = (unsigned)((n + CV_BLOCK - 1) / CV_BLOCK);
  if (reset) hipLaunchKernelGGL(k_curve_reset, dim3(blocks), dim3(CV_BLOCK), 0, stream, a);
  else hipLaunchKernelGGL(k_curve_fold, dim3(blocks), dim3(CV_BLOCK), 0, stream, a);
  if (hipError_t rc = hipGetLastError()) {
    *what = reset ? "k_curve_reset" : "k_curve_fold";
    *code = (int)rc;
    return -1;
  }
  return 0;
}

}  // namespace sfl
