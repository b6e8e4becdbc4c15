// The keyed-cell fold the learning curves, the exploit record and the policy bank share (DESIGN.md §17 states it;
// sfl_curve.h and sfl_eval.h hold the three layouts).  A cell is a few int64 words; a fold takes one contribution per
// env and step -- a cell of one episode or round -- and merges it into the cell its key names, word by word: a sum, a
// minimum or a maximum.  Every word is an integer, so the cells do not depend on the order contributions arrive in.
//
// A layout L states, once:  L::N  its words;  L::COUNT  the word that counts what was folded;  L::op(k)  word k's
// reduction;  L::identity(k)  the value an empty cell holds there (cell_op_identity(op(k)) unless the ABI says otherwise).
//
// The host build folds with cell_merge alone: in env order, one contribution at a time, no wave logic.  On the device
// (wave_fold) a wavefront reduces before it touches memory: per step it takes the first pending lane's key, ballots the
// lanes on the same key, reduces their words across the wavefront (lanes on another key contribute the identity) and
// lets one lane issue that cell's 64-bit integer atomics.  A lane alone on its key skips the reduction: such lanes
// issue their own atomics together after the loop.  Only vector loads and stores and global atomics.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SFL_CELL_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define SFL_CELL_FN inline
#endif

namespace sfl {

enum { OP_SUM = 0, OP_MIN = 1, OP_MAX = 2 };
SFL_CELL_FN constexpr int64_t cell_op_identity(int op) { return op == OP_MIN ? INT64_MAX : op == OP_MAX ? INT64_MIN : 0; }

// c = the empty cell: the identity of every word's reduction
template <class L>
SFL_CELL_FN void cell_clear(int64_t* c) {
  for (int k = 0; k < L::N; ++k) c[k] = L::identity(k);
}

// the contribution v folded into the cell c in memory
template <class L>
SFL_CELL_FN void cell_merge(int64_t* c, const int64_t* v) {
  for (int k = 0; k < L::N; ++k) {
    if (L::op(k) == OP_SUM) c[k] += v[k];
    else if (L::op(k) == OP_MIN) c[k] = v[k] < c[k] ? v[k] : c[k];
    else c[k] = v[k] > c[k] ? v[k] : c[k];
  }
}

// the host build's reset ("device" memory is host memory there)
template <class L>
inline void cells_reset_host(int64_t* cells, size_t n_cells) {
  for (size_t c = 0; c < n_cells; ++c) cell_clear<L>(cells + c * L::N);
}

#if defined(__HIPCC__)
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
template <class L>
__device__ __forceinline__ void cell_emit(int64_t* c, const int64_t (&v)[L::N]) {
#pragma unroll
  for (int k = 0; k < L::N; ++k) {
    if (L::op(k) == OP_SUM) {
      if (v[k] != 0) __hip_atomic_fetch_add(c + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (v[L::COUNT] != 0) {
      if (L::op(k) == OP_MIN) __hip_atomic_fetch_min(c + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else __hip_atomic_fetch_max(c + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// One step of a fold: every active lane holds one contribution v to the cell `key`; `pending` is the ballot of the
// active lanes (wave-uniform, as is every ballot below).  The distinct cells among them are taken one by one: the lanes
// on the first pending lane's cell are reduced across the wavefront and that lane issues the cell's atomics; a lane
// alone on its cell skips the reduction, and such lanes issue their own atomics together at the end.
template <class L>
__device__ __forceinline__ void wave_fold(int64_t* cells, uint32_t lane, bool active, uint64_t pending, uint32_t key,
                                          const int64_t (&v)[L::N]) {
  bool solo = false;
  while (pending) {
    const int leader = __ffsll((unsigned long long)pending) - 1;
    const uint32_t k0 = (uint32_t)__shfl((int)key, leader);
    const bool mine = active && key == k0;
    const uint64_t match = __ballot(mine);
    if (__popcll(match) == 1) {
      solo = solo || mine;
    } else {
      int64_t ident[L::N], r[L::N];
      cell_clear<L>(ident);
#pragma unroll
      for (int k = 0; k < L::N; ++k) {
        const int64_t x = mine ? v[k] : ident[k];
        r[k] = L::op(k) == OP_SUM ? wave_reduce<OP_SUM>(x) : L::op(k) == OP_MIN ? wave_reduce<OP_MIN>(x) : wave_reduce<OP_MAX>(x);
      }
      if ((int)lane == leader) cell_emit<L>(cells + (size_t)k0 * L::N, r);
    }
    pending &= ~match;
  }
  if (solo) cell_emit<L>(cells + (size_t)key * L::N, v);
}

// the body of a reset kernel, one lane per word: word i of n_words takes its identity
template <class L>
__device__ __forceinline__ void cells_reset(int64_t* cells, size_t i, size_t n_words) {
  if (i >= n_words) return;
  int64_t ident[L::N];
  cell_clear<L>(ident);
  int64_t x = 0;
#pragma unroll
  for (int k = 0; k < L::N; ++k) x = (int)(i % L::N) == k ? ident[k] : x;
  cells[i] = x;
}
#endif

}  // namespace sfl
