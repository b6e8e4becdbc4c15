// Consensus Q-tables on the device (include/sfl.h sfl_consensus; the rule: DESIGN.md "Consensus Q-tables").
//
// A streaming reduction over the members' Q blocks [E][Q] and a streaming broadcast back, in a translation unit of
// its own (it shares nothing with the wave kernels).  The unit of work is a *job*: one chunk of at most
// SFL_CONSENSUS_CHUNK members of one cohort (sfl_consensus.h ConsJob), times a tile of CONS_TILE consecutive cells.
// A block's lanes walk consecutive cells -- two per lane as one 16-byte access when the env stride Q is even (every
// env's block is then 16-byte aligned), one 8-byte access per lane when it is odd -- and its loop over the job's
// members keeps CONS_UNROLL loads per lane in flight, then accumulates them in member order.  A cohort of one chunk
// writes its consensus cells directly; a longer one writes a partial record per chunk (sum, first pattern, count,
// all-equal and held flags) and k_cons_combine folds the records in chunk order, so the bits do not depend on the grid.
// Only vector loads and stores; no atomics; a key-set word is read, OR-ed and written whole by one lane.
#include <hip/hip_runtime.h>

#include "sfl_consensus.h"

namespace {

using sfl::ConsArgs;
using sfl::ConsCombo;
using sfl::ConsJob;

constexpr int CONS_BLOCK = 256;
constexpr int CONS_UNROLL = 8;

template <int V>
struct Cells;
template <>
struct Cells<1> {
  double v[1];
  __device__ static Cells load(const double* p) { return Cells{{*p}}; }
};
template <>
struct Cells<2> {
  double v[2];
  __device__ static Cells load(const double* p) {
    const double2 t = *reinterpret_cast<const double2*>(p);
    return Cells{{t.x, t.y}};
  }
};

// per-cell accumulator of one chunk (MEAN: over the contributors; MAX: `first` is the best holder's pattern)
struct Acc {
  double sum = 0.0;
  uint64_t first = 0;
  uint32_t count = 0;
  bool eq = true, held = false;
};

template <int MODE>
__device__ __forceinline__ void acc_add(Acc& a, bool holds, double v, uint64_t dflt) {
  if (!holds) return;
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  if (MODE == SFL_CONSENSUS_MAX) {
    if (!a.held || v > __longlong_as_double((long long)a.first)) a.first = b;
  } else if (b != dflt) {
    if (a.count == 0) a.first = b;
    else if (b != a.first) a.eq = false;
    ++a.count;
    a.sum = a.sum + v;
  }
  a.held = true;
}

// the running combination of chunk records, in chunk order
struct Fold {
  double total = 0.0;
  uint64_t first = 0;
  uint32_t count = 0;
  bool eq = true, held = false;
};

template <int MODE>
__device__ __forceinline__ void fold_add(Fold& f, double sum, uint64_t first, uint32_t meta) {
  const uint32_t count = meta & sfl::CONS_M_COUNT;
  const bool held = (meta & sfl::CONS_M_HELD) != 0u;
  if (MODE == SFL_CONSENSUS_MAX) {
    if (held && (!f.held || __longlong_as_double((long long)first) > __longlong_as_double((long long)f.first)))
      f.first = first;
  } else {
    if (count) {
      if (f.count == 0) f.first = first;
      else if (first != f.first) f.eq = false;
      if (!(meta & sfl::CONS_M_EQ)) f.eq = false;
      f.count += count;
    }
    f.total = f.total + sum;
  }
  f.held = f.held || held;
}

template <int MODE>
__device__ __forceinline__ double fold_result(const Fold& f, uint64_t dflt) {
  if (MODE == SFL_CONSENSUS_MAX) return __longlong_as_double((long long)(f.held ? f.first : dflt));
  if (f.count == 0) return __longlong_as_double((long long)dflt);
  return f.eq ? __longlong_as_double((long long)f.first) : f.total / (double)f.count;
}

__device__ __forceinline__ uint32_t acc_meta(const Acc& a) {
  return a.count | (a.eq ? sfl::CONS_M_EQ : 0u) | (a.held ? sfl::CONS_M_HELD : 0u);
}

// key sets: one lane per (job, word) ORs the members' words; a one-chunk cohort's go to the consensus key set
__global__ void __launch_bounds__(CONS_BLOCK) k_cons_keys(ConsArgs a, uint32_t wtiles) {
  const ConsJob job = a.jobs[blockIdx.x / wtiles];
  const uint32_t w = (blockIdx.x % wtiles) * CONS_BLOCK + threadIdx.x;
  if (w >= a.tw) return;
  const uint32_t* mem = a.members + job.begin;
  uint32_t k = 0;
  for (uint32_t j = 0; j < job.n; ++j) k |= a.touched[(size_t)mem[j] * a.tw + w];
  if (job.slot == sfl::CONS_DIRECT) a.cons_keys[(size_t)job.cohort * a.tw + w] = k;
  else a.p_keys[(size_t)job.slot * a.tw + w] = k;
}

__global__ void __launch_bounds__(CONS_BLOCK) k_cons_keys_combine(ConsArgs a, uint32_t wtiles) {
  const ConsCombo cb = a.combos[blockIdx.x / wtiles];
  const uint32_t w = (blockIdx.x % wtiles) * CONS_BLOCK + threadIdx.x;
  if (w >= a.tw) return;
  uint32_t k = 0;
  for (uint32_t s = 0; s < cb.n_chunks; ++s) k |= a.p_keys[(size_t)(cb.slot0 + s) * a.tw + w];
  a.cons_keys[(size_t)cb.cohort * a.tw + w] = k;
}

// the reduction of one job over the cells [c0, c0 + tiles * CONS_TILE): V cells per lane
template <int MODE, int V>
__global__ void __launch_bounds__(CONS_BLOCK) k_cons_reduce(ConsArgs a, uint64_t c0, uint32_t tiles) {
  const ConsJob job = a.jobs[blockIdx.x / tiles];
  const uint64_t rel = ((uint64_t)(blockIdx.x % tiles) * CONS_BLOCK + threadIdx.x) * V;
  const uint64_t i0 = c0 + rel;
  if (i0 >= a.Q) return;  // (V == 2 only with an even Q: a pair is whole)
  uint32_t wi[V], sh[V];
  bool row[V];
#pragma unroll
  for (int c = 0; c < V; ++c) {
    const uint32_t r = a.cell_row[i0 + c];
    row[c] = r != sfl::CONS_NO_ROW;
    wi[c] = row[c] ? r >> 5 : 0u;
    sh[c] = r & 31u;
  }
  const bool same = V == 2 && wi[0] == wi[V - 1];
  const uint32_t* mem = a.members + job.begin;
  Acc acc[V];
  for (uint32_t j = 0; j < job.n; j += CONS_UNROLL) {
    Cells<V> v[CONS_UNROLL];
    uint32_t t[CONS_UNROLL][V];
#pragma unroll
    for (int u = 0; u < CONS_UNROLL; ++u)
      if (j + u < job.n) {
        const size_t e = mem[j + u];
        v[u] = Cells<V>::load(a.q + e * a.Q + i0);
        const uint32_t* tw = a.touched + e * a.tw;
        t[u][0] = tw[wi[0]];
        if (V == 2) t[u][V - 1] = same ? t[u][0] : tw[wi[V - 1]];
      }
#pragma unroll
    for (int u = 0; u < CONS_UNROLL; ++u)
      if (j + u < job.n) {
#pragma unroll
        for (int c = 0; c < V; ++c) acc_add<MODE>(acc[c], row[c] && ((t[u][c] >> sh[c]) & 1u), v[u].v[c], a.default_bits);
      }
  }
#pragma unroll
  for (int c = 0; c < V; ++c) {
    if (job.slot == sfl::CONS_DIRECT) {
      Fold f;
      fold_add<MODE>(f, acc[c].sum, acc[c].first, acc_meta(acc[c]));
      a.cons_q[(size_t)job.cohort * a.Q + i0 + c] = fold_result<MODE>(f, a.default_bits);
    } else {
      const size_t p = (size_t)job.slot * a.cells_cap + rel + c;
      a.p_sum[p] = acc[c].sum;
      a.p_first[p] = acc[c].first;
      a.p_meta[p] = acc_meta(acc[c]);
    }
  }
}

// a longer cohort's chunk records folded in chunk order: one cell per lane, two rounds per tile
template <int MODE>
__global__ void __launch_bounds__(CONS_BLOCK) k_cons_combine(ConsArgs a, uint64_t c0, uint32_t tiles) {
  const ConsCombo cb = a.combos[blockIdx.x / tiles];
  for (uint32_t k = 0; k < sfl::CONS_TILE / CONS_BLOCK; ++k) {
    const uint64_t rel = (uint64_t)(blockIdx.x % tiles) * sfl::CONS_TILE + k * CONS_BLOCK + threadIdx.x;
    if (c0 + rel >= a.Q) return;
    Fold f;
    for (uint32_t s = 0; s < cb.n_chunks; ++s) {
      const size_t p = (size_t)(cb.slot0 + s) * a.cells_cap + rel;
      fold_add<MODE>(f, a.p_sum[p], a.p_first[p], a.p_meta[p]);
    }
    a.cons_q[(size_t)cb.cohort * a.Q + c0 + rel] = fold_result<MODE>(f, a.default_bits);
  }
}

// SFL_CONSENSUS_SHARE: a job's tile of consensus cells, read once, written into every member of the job -- the cells
// of rows somebody holds only
template <int V>
__global__ void __launch_bounds__(CONS_BLOCK) k_cons_share(ConsArgs a, uint32_t tiles) {
  const ConsJob job = a.jobs[blockIdx.x / tiles];
  const uint64_t i0 = ((uint64_t)(blockIdx.x % tiles) * CONS_BLOCK + threadIdx.x) * V;
  if (i0 >= a.Q || job.n == 0) return;
  const uint32_t* keys = a.cons_keys + (size_t)job.cohort * a.tw;
  bool held[V];
#pragma unroll
  for (int c = 0; c < V; ++c) {
    const uint32_t r = a.cell_row[i0 + c];
    held[c] = r != sfl::CONS_NO_ROW && ((keys[r != sfl::CONS_NO_ROW ? r >> 5 : 0u] >> (r & 31u)) & 1u);
  }
  const Cells<V> v = Cells<V>::load(a.cons_q + (size_t)job.cohort * a.Q + i0);
  const uint32_t* mem = a.members + job.begin;
  if (V == 2 && held[0] && held[V - 1]) {
    const double2 both = make_double2(v.v[0], v.v[V - 1]);
    for (uint32_t j = 0; j < job.n; ++j) *reinterpret_cast<double2*>(a.q + (size_t)mem[j] * a.Q + i0) = both;
  } else {
#pragma unroll
    for (int c = 0; c < V; ++c)
      if (held[c])
        for (uint32_t j = 0; j < job.n; ++j) a.q[(size_t)mem[j] * a.Q + i0 + c] = v.v[c];
  }
}

__global__ void __launch_bounds__(CONS_BLOCK) k_cons_share_keys(ConsArgs a, uint32_t wtiles) {
  const ConsJob job = a.jobs[blockIdx.x / wtiles];
  const uint32_t w = (blockIdx.x % wtiles) * CONS_BLOCK + threadIdx.x;
  if (w >= a.tw) return;
  const uint32_t k = a.cons_keys[(size_t)job.cohort * a.tw + w];
  if (!k) return;
  const uint32_t* mem = a.members + job.begin;
  for (uint32_t j = 0; j < job.n; ++j) {
    uint32_t* t = a.touched + (size_t)mem[j] * a.tw + w;
    const uint32_t old = *t;
    if ((old | k) != old) *t = old | k;
  }
}

}  // namespace

namespace sfl {

LaunchErr consensus_launch(const ConsArgs& a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint64_t kMaxGrid = 0x7FFFFFFFull;
  const uint32_t wtiles = (a.tw + CONS_BLOCK - 1) / CONS_BLOCK;
  const uint64_t all_tiles = (a.Q + CONS_TILE - 1) / CONS_TILE;
  const bool mx = a.mode == SFL_CONSENSUS_MAX, v2 = (a.Q & 1ull) == 0;
  // (a lane of the two-cell kernels covers CONS_TILE / CONS_BLOCK = 2 cells; the one-cell kernels take two blocks per tile)
  const uint32_t per = v2 ? 1u : CONS_TILE / CONS_BLOCK;
  if ((uint64_t)a.n_jobs * all_tiles * per > kMaxGrid || (uint64_t)a.n_jobs * wtiles > kMaxGrid)
    return launch_err("sfl_consensus: more than 2^31 blocks (jobs x cell tiles)", hipErrorInvalidConfiguration);
  hipLaunchKernelGGL(k_cons_keys, dim3(a.n_jobs * wtiles), dim3(CONS_BLOCK), 0, stream, a, wtiles);
  if (a.n_combos)
    hipLaunchKernelGGL(k_cons_keys_combine, dim3(a.n_combos * wtiles), dim3(CONS_BLOCK), 0, stream, a, wtiles);
  if (LaunchErr e = launch_err("k_cons_keys")) return e;
  // (cells_cap covers the table: one pass; a smaller cells_cap would reduce it a range of cells at a time)
  const uint64_t step = a.cells_cap;
  for (uint64_t c0 = 0; c0 < a.Q; c0 += step) {
    const uint64_t cells = a.Q - c0 < step ? a.Q - c0 : step;
    const uint32_t tiles = (uint32_t)((cells + CONS_TILE - 1) / CONS_TILE);
    const dim3 grid(a.n_jobs * tiles * per);
    if (v2) {
      if (mx) hipLaunchKernelGGL((k_cons_reduce<SFL_CONSENSUS_MAX, 2>), grid, dim3(CONS_BLOCK), 0, stream, a, c0, tiles * per);
      else hipLaunchKernelGGL((k_cons_reduce<SFL_CONSENSUS_MEAN, 2>), grid, dim3(CONS_BLOCK), 0, stream, a, c0, tiles * per);
    } else {
      if (mx) hipLaunchKernelGGL((k_cons_reduce<SFL_CONSENSUS_MAX, 1>), grid, dim3(CONS_BLOCK), 0, stream, a, c0, tiles * per);
      else hipLaunchKernelGGL((k_cons_reduce<SFL_CONSENSUS_MEAN, 1>), grid, dim3(CONS_BLOCK), 0, stream, a, c0, tiles * per);
    }
    if (LaunchErr e = launch_err("k_cons_reduce")) return e;
    if (a.n_combos) {
      if (mx) hipLaunchKernelGGL(k_cons_combine<SFL_CONSENSUS_MAX>, dim3(a.n_combos * tiles), dim3(CONS_BLOCK), 0, stream, a, c0, tiles);
      else hipLaunchKernelGGL(k_cons_combine<SFL_CONSENSUS_MEAN>, dim3(a.n_combos * tiles), dim3(CONS_BLOCK), 0, stream, a, c0, tiles);
      if (LaunchErr e = launch_err("k_cons_combine")) return e;
    }
  }
  if (a.flags & SFL_CONSENSUS_SHARE) {
    const uint32_t tiles = (uint32_t)(all_tiles * per);
    if (v2) hipLaunchKernelGGL(k_cons_share<2>, dim3(a.n_jobs * tiles), dim3(CONS_BLOCK), 0, stream, a, tiles);
    else hipLaunchKernelGGL(k_cons_share<1>, dim3(a.n_jobs * tiles), dim3(CONS_BLOCK), 0, stream, a, tiles);
    hipLaunchKernelGGL(k_cons_share_keys, dim3(a.n_jobs * wtiles), dim3(CONS_BLOCK), 0, stream, a, wtiles);
    if (LaunchErr e = launch_err("k_cons_share")) return e;
  }
  return {};
}

}  // namespace sfl
