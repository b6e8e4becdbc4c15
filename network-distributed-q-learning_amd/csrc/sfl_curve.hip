// Step-mode learning curves on the device (include/sfl.h sfl_curve_*; the rule: DESIGN.md §17).
//
// k_curve_fold reduces the statistics rows a step launch wrote into the handle's ring into the (bin, series) cells, in
// a translation unit of its own (it shares nothing with the wave kernels).  One lane per env: the lanes of a wavefront
// read consecutive envs of the [row][E] ring arrays (the T delay rows [(row * T + h) * E + e] too), each lane walks its
// own finished episodes and the wavefront loops to its longest lane.  Nearly every env of a launch lands in the same
// one or two cells, so each step of the loop goes through the keyed-cell fold of sfl_cells.h (wave_fold: the wavefront
// reduces before it touches memory; a lane alone on its cell -- one series per env -- issues its own atomics).
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

__global__ void __launch_bounds__(CV_BLOCK) k_curve_fold(CurveArgs a) {
  const uint32_t e = blockIdx.x * CV_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const bool in = e < a.E;
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
    sfl::cell_clear<sfl::EpisodeCell>(v);  // the identity of every word's reduction
    uint32_t key = 0xFFFFFFFFu;
    if (active) sfl::curve_episode_cell(a, e, ser, i, kept, v, key);
    sfl::wave_fold<sfl::EpisodeCell>(a.cells, lane, active, pending, key, v);
  }
  if (in) a.mark[e] = end;
}

// the cells emptied (sfl_curve_begin, sfl_learn_begin): one lane per word
__global__ void __launch_bounds__(CV_BLOCK) k_curve_reset(CurveArgs a) {
  sfl::cells_reset<sfl::EpisodeCell>(a.cells, (size_t)blockIdx.x * CV_BLOCK + threadIdx.x, (size_t)a.n_bins * a.n_series * CV_WORDS);
}

// The exploit record's fold (include/sfl.h sfl_curve_exploit): one lane per env reads its episode index,
// flags word, mark and series (consecutive envs: coalesced), counts the greedy rounds the env has completed and walks
// the ones since its mark -- step k of the loop is round mark + k, read from ring row t_r % ring_cap of the two
// [row][E] arrays the kernels write at a round's end.  The same reduction per step as k_curve_fold (wave_fold).
__global__ void __launch_bounds__(CV_BLOCK) k_curve_fold_exploit(CurveXArgs a) {
  const uint32_t e = blockIdx.x * CV_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const bool in = e < a.E;
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
    sfl::cell_clear<sfl::ExploitCell>(v);
    uint32_t key = 0xFFFFFFFFu;
    if (active) sfl::curve_round_cell(a, e, ser, r, kept, v, key);
    sfl::wave_fold<sfl::ExploitCell>(a.cells, lane, active, pending, key, v);
  }
  if (in) a.mark[e] = n;
}

__global__ void __launch_bounds__(CV_BLOCK) k_curve_reset_exploit(CurveXArgs a) {
  sfl::cells_reset<sfl::ExploitCell>(a.cells, (size_t)blockIdx.x * CV_BLOCK + threadIdx.x, (size_t)a.n_bins * a.n_series * XV_WORDS);
}

}  // namespace

namespace sfl {

LaunchErr curve_launch(const CurveArgs& a, bool reset, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const size_t n = reset ? (size_t)a.n_bins * a.n_series * CV_WORDS : (size_t)a.E;
  const unsigned blocks = (unsigned)((n + CV_BLOCK - 1) / CV_BLOCK);
  if (reset) hipLaunchKernelGGL(k_curve_reset, dim3(blocks), dim3(CV_BLOCK), 0, stream, a);
  else hipLaunchKernelGGL(k_curve_fold, dim3(blocks), dim3(CV_BLOCK), 0, stream, a);
  return launch_err(reset ? "k_curve_reset" : "k_curve_fold");
}

LaunchErr curve_xlaunch(const CurveXArgs& a, bool reset, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const size_t n = reset ? (size_t)a.n_bins * a.n_series * XV_WORDS : (size_t)a.E;
  const unsigned blocks = (unsigned)((n + CV_BLOCK - 1) / CV_BLOCK);
  if (reset) hipLaunchKernelGGL(k_curve_reset_exploit, dim3(blocks), dim3(CV_BLOCK), 0, stream, a);
  else hipLaunchKernelGGL(k_curve_fold_exploit, dim3(blocks), dim3(CV_BLOCK), 0, stream, a);
  return launch_err(reset ? "k_curve_reset_exploit" : "k_curve_fold_exploit");
}

}  // namespace sfl
