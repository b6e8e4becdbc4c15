// External-action mode's transition assembler on the device (include/sfl.h sfl_env_trans_*; the rules and the per-env
// logic: sfl_trans.h).  A translation unit of its own: it reads what the env step wrote and shares
// nothing else with the step kernels.  Two kernels behind every env step, a lane per env, TRANS_BLOCK envs per block:
//   k_trans_count  each env's rows of this call into cnt[e], each block's sum into blk[b].  Nothing else is written.
//   k_trans_write  every block sums blk[0 .. b) and blk[0 .. nb) itself (nb = ceil(E / 256): 256 integers at 65,536
//                  envs), scans its envs' counts (a shuffle scan per wavefront, the four wavefront sums through LDS),
//                  and so knows each row's rank in the call and with it its ring slot: no atomics, no block waits for
//                  another, and the order does not depend on scheduling.  Then the rows, then the envs' own state.
// Step 1's rows (almost every env has one) go through LDS: a lane puts its row's words there, and the block writes the
// columns with consecutive threads on consecutive addresses -- a thread per 8-byte obs pair, as k_env_encode does.
// Step 3's rows are rare: the wavefront takes the envs with a newly arrived train one at a time and reads the train's
// S entries together (64 entries of 16 bytes per load, one ballot each); a lane that finds a live entry writes its row.
// The cursor (total, total % N) is double-buffered: a call reads one copy and block 0 writes the other, so no block
// can see the advanced value.  Only vector loads and stores.
#include <hip/hip_runtime.h>

#include "sfl_trans.h"

namespace {

using sfl::TransArgs;
using sfl::TransEntry;
using sfl::TransEnv;
using sfl::TransRow;
using sfl::TransScan;

constexpr int BLOCK = sfl::TRANS_BLOCK;
constexpr int WAVES = BLOCK / 64;

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
  return (uint64_t)hi << 32 | lo;
}

// step 3 for the envs of this wavefront that have a newly arrived train, one env at a time, all 64 lanes on its table.
// Returns, in the env's own lane, the rows it found.  WRITE: the rows go out (rank: the env's first such row in the
// call) and their entries are cleared
template <bool WRITE>
__device__ __forceinline__ uint32_t walk_arrivals(const TransArgs& a, const TransEnv& v, uint32_t e, uint32_t lane,
                                                  uint64_t rank, uint64_t skip, uint64_t head, bool over) {
  uint32_t mine = 0u;
  uint64_t todo = __ballot(v.any_fresh);
  const uint64_t below = (1ull << lane) - 1ull;
  while (todo) {
    const int src = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1ull;
    TransScan c;
    c.e = __shfl(e, src);
    c.epoch = __shfl(v.epoch, src);
    c.h = __shfl(v.p.train, src);
    c.s = __shfl(v.p.agent, src);
    c.nsw = __shfl(v.nsw, src);
    const TransEntry made = sfl::trans_made(v);
    c.made.who = __shfl(made.who, src);
    c.made.state = __shfl(made.state, src);
    c.made.now = __shfl(made.now, src);
    c.made.stamp = c.epoch + 1u;
    const uint64_t first = WRITE ? shfl64(rank, src) : 0ull;
    uint32_t n = 0u;
#pragma unroll
    for (int w = 0; w < sfl::MAXW; ++w) {
      uint32_t f = __shfl(v.fresh[w], src);
      while (f) {
        const int tr = w * 32 + __ffs(f) - 1;
        f &= f - 1u;
        for (int b0 = 0; b0 < a.S; b0 += 64) {
          const int sw = b0 + (int)lane;
          const bool in = sw < a.S;
          const size_t ix = sfl::trans_ix(a, c.e, tr, in ? sw : 0);
          TransEntry x{0u, 0u, 0, 0u};
          if (in) x = a.tab[ix];
          const bool on = in && sfl::trans_live(c, tr, sw, x);
          const uint64_t bal = __ballot(on);
          if (WRITE && on) {
            const uint64_t r = first + n + (uint32_t)__popcll(bal & below);
            if (r >= skip) {
              TransRow row = sfl::trans_row_bonus(x, c.e, tr);
              row.slot = sfl::trans_slot(head, r, a.N, over);
              sfl::trans_store_row(a, row);
            }
            a.tab[ix].stamp = 0u;
          }
          n += (uint32_t)__popcll(bal);
        }
      }
    }
    if ((int)lane == src) mine = n;
  }
  return mine;
}

__global__ void __launch_bounds__(BLOCK) k_trans_count(const TransArgs a) {
  __shared__ uint32_t wsum[WAVES];
  const uint32_t t = threadIdx.x, lane = t & 63u, e = blockIdx.x * BLOCK + t;
  TransEnv v{};
  if (e < a.E) sfl::trans_env_head(a, e, v);
  uint32_t n = v.consumed ? 1u : 0u;
  n += walk_arrivals<false>(a, v, e, lane, 0ull, 0ull, 0ull, false);
  if (e < a.E) a.cnt[e] = n;
  uint32_t s = n;
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  if (lane == 0u) wsum[t >> 6] = s;
  __syncthreads();
  if (t == 0u) {
    uint32_t b = 0u;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) b += wsum[w];
    a.blk[blockIdx.x] = b;
  }
}

__global__ void __launch_bounds__(BLOCK) k_trans_write(const TransArgs a, uint32_t nb) {
  __shared__ TransRow rows[BLOCK];
  __shared__ uint64_t red[2][WAVES];
  __shared__ uint32_t wsum[WAVES], wrow[WAVES];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6, e = blockIdx.x * BLOCK + t;
  const uint64_t below = (1ull << lane) - 1ull;
  TransEnv v{};
  if (e < a.E) sfl::trans_env_head(a, e, v);
  const uint32_t n = e < a.E ? a.cnt[e] : 0u;
  // the blocks' sums: those before this block, and all of them
  uint64_t before = 0ull, all = 0ull;
  for (uint32_t i = t; i < nb; i += BLOCK) {
    const uint32_t c = a.blk[i];
    all += c;
    before += i < blockIdx.x ? c : 0u;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    before += shfl64(before, (int)(lane ^ (uint32_t)d));
    all += shfl64(all, (int)(lane ^ (uint32_t)d));
  }
  // this block's envs: an inclusive scan of the counts per wavefront
  uint32_t inc = n;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d);
    inc += lane >= (uint32_t)d ? up : 0u;
  }
  if (lane == 0u) {
    red[0][wv] = before;
    red[1][wv] = all;
  }
  if (lane == 63u) wsum[wv] = inc;
  __syncthreads();
  before = all = 0ull;
  uint32_t off = 0u;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    before += red[0][w];
    all += red[1][w];
    off += (uint32_t)w < wv ? wsum[w] : 0u;
  }
  const uint64_t total = a.cur[2u * a.parity], head = a.cur[2u * a.parity + 1u];
  const bool over = all > a.N;
  const uint64_t skip = over ? all - a.N : 0ull;
  const uint64_t rank = before + off + (inc - n);  // of the env's first row in the call
  // step 1's rows that are written, packed into LDS in env order
  const bool put = v.consumed && rank >= skip;
  const uint64_t bal = __ballot(put);
  if (lane == 0u) wrow[wv] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t at = (uint32_t)__popcll(bal & below), nrows = 0u;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    at += (uint32_t)w < wv ? wrow[w] : 0u;
    nrows += wrow[w];
  }
  if (put) {
    TransRow r = sfl::trans_row_next(v, e);
    r.slot = sfl::trans_slot(head, rank, a.N, over);
    rows[at] = r;
  }
  __syncthreads();
  for (uint32_t i = t; i < nrows; i += BLOCK) sfl::trans_store_scalars(a, rows[i]);
  if (a.r_obs)
    for (uint32_t i = t; i < nrows * (uint32_t)sfl::OBS_PAIRS; i += BLOCK)
      sfl::trans_store_pair(a, rows[i / sfl::OBS_PAIRS], i % sfl::OBS_PAIRS);
  if (a.r_next_obs)
    for (uint32_t i = t; i < nrows * (uint32_t)sfl::OBS_PAIRS; i += BLOCK)
      sfl::trans_store_pair(a, rows[i / sfl::OBS_PAIRS], sfl::OBS_PAIRS + i % sfl::OBS_PAIRS);
  // every table word an env's own lane read is in its registers before another lane clears entries of that env
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  walk_arrivals<true>(a, v, e, lane, rank + (v.consumed ? 1u : 0u), skip, head, over);
  if (e < a.E) sfl::trans_env_tail(a, e, v, n);
  if (blockIdx.x == 0u && t == 0u) {
    uint64_t* nxt = a.cur + 2u * (1u - a.parity);
    nxt[0] = total + all;
    nxt[1] = (head + all) % a.N;
    *a.total = (int64_t)(total + all);
    *a.last_count = (int32_t)all;
  }
}

}  // namespace

namespace sfl {

LaunchErr trans_launch(const TransArgs& a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const uint32_t nb = (a.E + TRANS_BLOCK - 1) / TRANS_BLOCK;
  hipLaunchKernelGGL(k_trans_count, dim3(nb), dim3(TRANS_BLOCK), 0, stream, a);
  if (LaunchErr e = launch_err("k_trans_count")) return e;
  hipLaunchKernelGGL(k_trans_write, dim3(nb), dim3(TRANS_BLOCK), 0, stream, a, nb);
  return launch_err("k_trans_write");
}

}  // namespace sfl
