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
// k_curve_fold_exploit folds the greedy rounds of a handle with an exploit record (sfl_curve_exploit)
// the same way, into cells of 11 words.
// Only vector loads and stores and global atomics.
#include <hip/hip_runtime.h>

#include "sfl_curve.h"

namespace {

using sfl::CurveArgs;
using sfl::CurveXArgs;
using sfl::CV_WORDS;
using sfl::XV_WORDS;

constexpr int CV_BLOCK = 256;

enum { OP_SUM = 0, OP_MIN = 1, OP_MAX = 2 };
// the two cell layouts: their words, the word that says "something was folded", each word's reduction, the identity
struct EpisodeCell {
  static constexpr int N = CV_WORDS, COUNT = sfl::CV_COUNT;
  __host__ __device__ static constexpr int op(int k) {
    return (k == sfl::CV_ARR_MIN || k == sfl::CV_REW_MIN || k == sfl::CV_EP_FIRST) ? OP_MIN
           : (k == sfl::CV_ARR_MAX || k == sfl::CV_REW_MAX || k == sfl::CV_EP_LAST) ? OP_MAX
                                                                                    : OP_SUM;
  }
  __host__ __device__ static void clear(int64_t* c) { sfl::curve_cell_clear(c); }
};
struct ExploitCell {
  static constexpr int N = XV_WORDS, COUNT = sfl::XV_COUNT;
  __host__ __device__ static constexpr int op(int k) {
    return (k == sfl::XV_ARR_MIN || k == sfl::XV_REW_MIN || k == sfl::XV_EP_FIRST) ? OP_MIN
           : (k == sfl::XV_ARR_MAX || k == sfl::XV_REW_MAX || k == sfl::XV_EP_LAST) ? OP_MAX
                                                                                    : OP_SUM;
  }
  __host__ __device__ static void clear(int64_t* c) { sfl::curve_xcell_clear(c); }
};

template <int OP>
__device__ __forceinline__ int64_t wave_reduce(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t w = (int64_t)__shfl_xor((long long)v, o);
    v = OP == OP_SUM ? v + w : OP == OP_MIN ? (w < v ? w : v) : (w > v ? w : v);
  }
  return v;
}

// one cell's words into memory: the sums that are not zero; min / max only when something was folded
template <class Cell>
__device__ __forceinline__ void emit(int64_t* c, const int64_t (&v)[Cell::N]) {
#pragma unroll
  for (int k = 0; k < Cell::N; ++k) {
    if (Cell::op(k) == OP_SUM) {
      if (v[k] != 0) __hip_atomic_fetch_add(c + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (v[Cell::COUNT] != 0) {
      if (Cell::op(k) == OP_MIN) __hip_atomic_fetch_min(c + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else __hip_atomic_fetch_max(c + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// One step of a fold: every active lane holds one contribution v to the cell `key`; `pending` is the ballot of the
// active lanes (wave-uniform, as is every ballot below).  The distinct cells among them are taken one by one: the lanes
// on the first pending lane's cell are reduced across the wavefront and that lane issues the cell's atomics; a lane
// alone on its cell skips the reduction, and such lanes issue their own atomics together at the end.
template <class Cell>
__device__ __forceinline__ void wave_fold(int64_t* cells, uint32_t lane, bool active, uint64_t pending, uint32_t key,
                                          const int64_t (&v)[Cell::N]) {
  bool solo = false;
  while (pending) {
    const int leader = __ffsll((unsigned long long)pending) - 1;
    const uint32_t k0 = (uint32_t)__shfl((int)key, leader);
    const bool mine = active && key == k0;
    const uint64_t match = __ballot(mine);
    if (__popcll(match) == 1) {
      solo = solo || mine;
    } else {
      int64_t ident[Cell::N], r[Cell::N];
      Cell::clear(ident);
#pragma unroll
      for (int k = 0; k < Cell::N; ++k) {
        const int64_t x = mine ? v[k] : ident[k];
        r[k] = Cell::op(k) == OP_SUM ? wave_reduce<OP_SUM>(x) : Cell::op(k) == OP_MIN ? wave_reduce<OP_MIN>(x) : wave_reduce<OP_MAX>(x);
      }
      if ((int)lane == leader) emit<Cell>(cells + (size_t)k0 * Cell::N, r);
    }
    pending &= ~match;
  }
  if (solo) emit<Cell>(cells + (size_t)key * Cell::N, v);
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
    wave_fold<EpisodeCell>(a.cells, lane, active, pending, key, v);
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

// The exploit record's fold (include/sfl.h sfl_curve_exploit): one lane per env reads its episode index,
// flags word, mark and series (consecutive envs: coalesced), counts the greedy rounds the env has completed and walks
// the ones since its mark -- step k of the loop is round mark + k, read from ring row t_r % ring_cap of the two
// [row][E] arrays the kernels write at a round's end.  The same reduction per step as k_curve_fold (wave_fold).
__global__ void __launch_bounds__(CV_BLOCK) k_curve_fold_exploit(CurveXArgs a) {
  const uint32_t e = blockIdx.x * CV_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const bool in = e < a.E;
  const size_t E = a.E;
  int32_t b = 0, n = 0;
  uint32_t ser = 0;
  if (in) {
    n = sfl::curve_rounds_done(a.ep_t[e], a.eflags[e], a.f);
    if (a.limit) {  // (wave-uniform: a kernel argument) no round starts any more
      const int32_t most = a.limit[e];
      n = most < n ? most : n;
    }
    b = a.mark[e];
    ser = a.series[e];
  }
  const int32_t kept = n - a.period > b ? n - a.period : b;  // the rounds below it were overwritten
  for (int32_t r = b;; ++r) {
    const bool active = in && r < n;
    const uint64_t pending = __ballot(active);
    if (!pending) break;
    int64_t v[XV_WORDS];
    sfl::curve_xcell_clear(v);
    uint32_t key = 0xFFFFFFFFu;
    if (active) {
      const int32_t t = sfl::curve_round_episode(r, a.f);
      key = (uint32_t)sfl::curve_xcell_of(a, t, ser);
      if (r < kept) {
        v[sfl::XV_LOST] = 1;
      } else {
        const size_t row = (size_t)(t % a.ring_cap);
        const int64_t arrived = a.sx_arrived[row * E + e], reward = (int64_t)a.sx_cum[row * E + e];
        v[sfl::XV_COUNT] = 1;
        v[sfl::XV_ARR_SUM] = v[sfl::XV_ARR_MIN] = v[sfl::XV_ARR_MAX] = arrived;
        v[sfl::XV_ALL_ARR] = arrived == a.T ? 1 : 0;
        v[sfl::XV_REW_SUM] = v[sfl::XV_REW_MIN] = v[sfl::XV_REW_MAX] = reward;
        v[sfl::XV_EP_FIRST] = v[sfl::XV_EP_LAST] = t;
      }
    }
    wave_fold<ExploitCell>(a.cells, lane, active, pending, key, v);
  }
  if (in) a.mark[e] = n;
}

__global__ void __launch_bounds__(CV_BLOCK) k_curve_reset_exploit(CurveXArgs a) {
  const size_t i = (size_t)blockIdx.x * CV_BLOCK + threadIdx.x;
  if (i >= (size_t)a.n_bins * a.n_series * XV_WORDS) return;
  int64_t ident[XV_WORDS];
  sfl::curve_xcell_clear(ident);
  int64_t x = 0;
#pragma unroll
  for (int k = 0; k < XV_WORDS; ++k) x = (int)(i % XV_WORDS) == k ? ident[k] : x;
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

int curve_xlaunch(const CurveXArgs& a, bool reset, void* stream_, const char** what, int* code) {
  hipStream_t stream = (hipStream_t)stream_;
  const size_t n = reset ? (size_t)a.n_bins * a.n_series * XV_WORDS : (size_t)a.E;
  const unsigned blocks = (unsigned)((n + CV_BLOCK - 1) / CV_BLOCK);
  if (reset) hipLaunchKernelGGL(k_curve_reset_exploit, dim3(blocks), dim3(CV_BLOCK), 0, stream, a);
  else hipLaunchKernelGGL(k_curve_fold_exploit, dim3(blocks), dim3(CV_BLOCK), 0, stream, a);
  if (hipError_t rc = hipGetLastError()) {
    *what = reset ? "k_curve_reset_exploit" : "k_curve_fold_exploit";
    *code = (int)rc;
    return -1;
  }
  return 0;
}

}  // namespace sfl
