// Policy-bank evaluation, the traffic fold of a recording on the device (include/sfl.h sfl_bank_record_traffic;
// DESIGN.md §28), in a translation unit of its own (it shares nothing with the wave kernels).  Two launches on the
// handle's stream: k_rec_reset empties the output words, k_rec_traffic reduces the recorded frames and decision rows of
// the slots whose env followed the asked policy (the rule: include/sfl.h; its per-word function: sfl_rec.h).
//
// k_rec_traffic's mapping.  Block (k, y) takes slot k's frame words [y * RC_CHUNK, (y + 1) * RC_CHUNK) of the kept
// ones -- a slot's frames are one run of kept_ticks * T words per array, so the block's threads read consecutive words
// (and the word T before each, the train's cell one tick earlier: the same lines again).  A block whose slot follows
// another policy, or whose chunk lies past the kept frames, leaves at once (both tests are block-uniform, and stand in
// front of every barrier).  The three per-cell counts are taken in the block's LDS when 3 * H * W words fit
// (RC_LDS_WORDS: maps up to 4,096 cells) and flushed with one global atomic per non-zero word; on larger maps every
// frame word issues its global atomics directly.  Blocks y = 0 also take their slot's decision rows, one row per thread
// and step, with global atomics on the per-switch counts.  Every word is an integer sum: the result does not depend on
// the order.  Only vector loads and stores, LDS atomics and global atomics.
#include <hip/hip_runtime.h>

#include "sfl_rec.h"

namespace {

using sfl::RecArgs;

constexpr int RC_BLOCK = 256;
constexpr int RC_CHUNK = RC_BLOCK * 32;  // frame words of a block
constexpr int RC_LDS_WORDS = 12288;      // 48 KB

template <bool LDS>
__device__ __forceinline__ void rec_frames(const RecArgs& a, uint32_t* hist, size_t base, size_t w0, size_t w1) {
  const size_t HW = a.HW;
  if constexpr (LDS) {
    for (size_t i = threadIdx.x; i < 3 * HW; i += RC_BLOCK) hist[i] = 0u;
    __syncthreads();
  }
  for (size_t w = w0 + threadIdx.x; w < w1; w += RC_BLOCK) {
    int32_t c;
    const uint32_t r = sfl::rec_frame_word(a, base, w, c);
    if constexpr (LDS) {
      if (r & 1u) atomicAdd(&hist[c], 1u);
      if (r & 2u) atomicAdd(&hist[HW + c], 1u);
      if (r & 4u) atomicAdd(&hist[2 * HW + c], 1u);
    } else {
      if (r & 1u) atomicAdd(a.out + c, 1u);
      if (r & 2u) atomicAdd(a.out + HW + c, 1u);
      if (r & 4u) atomicAdd(a.out + 2 * HW + c, 1u);
    }
  }
  if constexpr (LDS) {
    __syncthreads();
    for (size_t i = threadIdx.x; i < 3 * HW; i += RC_BLOCK) {
      const uint32_t v = hist[i];
      if (v) atomicAdd(a.out + i, v);
    }
  }
}

__global__ void __launch_bounds__(RC_BLOCK) k_rec_traffic(RecArgs a) {
  __shared__ uint32_t hist[RC_LDS_WORDS];
  const uint32_t k = blockIdx.x;  // (k < n: the grid)
  const uint32_t e = a.env[k];    // (e < E: sfl_bank_record checked it)
  if (a.policy[e] != a.p) return;
  const size_t HW = a.HW;
  if (blockIdx.y == 0) {
    const int32_t* rows = a.rows + (size_t)k * (size_t)a.dec_cap * sfl::RC_DEC_WORDS;
    const int32_t nd = sfl::rec_kept(a.dec[e], a.dec_cap);
    for (int32_t d = (int32_t)threadIdx.x; d < nd; d += RC_BLOCK) {
      const uint32_t sw = (uint32_t)rows[(size_t)d * sfl::RC_DEC_WORDS + sfl::RC_SWITCH];
      if (sw >= a.S) continue;
      atomicAdd(a.out + 3 * HW + sw, 1u);
      if (rows[(size_t)d * sfl::RC_DEC_WORDS + sfl::RC_ACTION] == (int32_t)a.sw_na[sw] - 1) atomicAdd(a.out + 3 * HW + a.S + sw, 1u);
    }
  }
  const size_t nw = (size_t)sfl::rec_kept(a.ticks[e], a.tick_cap) * (size_t)a.T;
  const size_t w0 = (size_t)blockIdx.y * RC_CHUNK;
  if (w0 >= nw) return;
  const size_t w1 = w0 + RC_CHUNK < nw ? w0 + RC_CHUNK : nw;
  const size_t base = (size_t)k * (size_t)a.tick_cap * (size_t)a.T;
  if (3 * HW <= (size_t)RC_LDS_WORDS) rec_frames<true>(a, hist, base, w0, w1);
  else rec_frames<false>(a, hist, base, w0, w1);
}

__global__ void __launch_bounds__(RC_BLOCK) k_rec_reset(uint32_t* out, size_t n_words) {
  const size_t i = (size_t)blockIdx.x * RC_BLOCK + threadIdx.x;
  if (i < n_words) out[i] = 0u;
}

}  // namespace

namespace sfl {

LaunchErr rec_traffic_launch(const RecArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t n_words = 3 * (size_t)a.HW + 2 * (size_t)a.S;
  k_rec_reset<<<(unsigned)((n_words + RC_BLOCK - 1) / RC_BLOCK), RC_BLOCK, 0, st>>>(a.out, n_words);
  if (LaunchErr e = launch_err("k_rec_reset")) return e;
  if (a.n == 0) return LaunchErr{};
  const size_t words = (size_t)a.tick_cap * (size_t)a.T;
  const unsigned gy = (unsigned)((words + RC_CHUNK - 1) / RC_CHUNK);
  k_rec_traffic<<<dim3(a.n, gy ? gy : 1u), RC_BLOCK, 0, st>>>(a);
  return launch_err("k_rec_traffic");
}

}  // namespace sfl
