// Suspend and resume on the device (include/sfl.h sfl_state_*; the format and the live-row rule: sfl_snap.h).
//
// A translation unit of its own (it shares nothing with the step kernels).  The unit of work of the Q passes is a row:
// lane i of a block takes row blockIdx * 256 + i of one listed env, so a wavefront covers one SNAP_GROUP of 64
// consecutive rows, whose cells are consecutive in the env's block (a row is 1 - 4 cells: the lanes' loads of column j
// are q_w * 8 bytes apart and together cover every byte of the lines they touch once).
//   count:   k_snap_live<true> reads the rows, ballots "key bit set or a cell differs from default_q" into the env's
//            live bitmap and writes each group's row and cell counts; k_snap_scan_env (a block per env) turns them into
//            exclusive prefixes and the env's totals; k_snap_scan_all (one block, any n) into row_off / cell_off.
//   gather:  k_snap_rows<true> ranks a live row inside its group by popcounts of the ballot below its lane, adds the
//            group's and the env's prefixes and writes its id and cells; k_snap_field<true> copies every state array's
//            slice, and the key sets, into the records.
//   restore: k_snap_fill, k_snap_live<false> on the bitmap the host built from the record's row ids, the same scan,
//            k_snap_rows<false> and k_snap_field<false>.
// The output order depends on row ids and list positions alone, never on block scheduling.  Only vector loads and
// stores; no atomics.
#include <hip/hip_runtime.h>

#include "sfl_snap.h"

namespace {

using sfl::SnapArgs;
using sfl::SnapField;

constexpr int SNAP_BLOCK = 256;
static_assert(sfl::SNAP_GROUP == 64, "a scan group is one wavefront's ballot");

__device__ __forceinline__ uint32_t cells_of(uint64_t b0, uint64_t b1, uint64_t b2) {
  return (uint32_t)__popcll(b0) + 2u * (uint32_t)__popcll(b1) + 4u * (uint32_t)__popcll(b2);
}

// FROM_Q: the live rule on the env's block and key set, into the bitmap; else the bitmap as given.  Either way each
// group's live rows and their cells.
template <bool FROM_Q>
__global__ void __launch_bounds__(SNAP_BLOCK) k_snap_live(SnapArgs a, uint32_t rblocks) {
  const uint32_t k = blockIdx.x / rblocks;
  const uint32_t r = (blockIdx.x % rblocks) * SNAP_BLOCK + threadIdx.x;
  const size_t e = a.envs[k];
  const bool valid = r < a.rows;
  const uint32_t w = valid ? a.row_w[r] : 0u;
  bool on;
  if (FROM_Q) {
    on = valid && ((a.touched[e * a.tw + (r >> 5)] >> (r & 31u)) & 1u);
    if (w) {
      const uint64_t* p = a.q + e * a.Q + a.row_cell[r];
      for (uint32_t j = 0; j < w; ++j) on = on || p[j] != a.default_bits;
    }
  } else {
    on = valid && ((a.live[(size_t)k * a.tw + (r >> 5)] >> (r & 31u)) & 1u);
  }
  const uint32_t lw = on ? w : 0u;
  const uint64_t bal = __ballot(on), b0 = __ballot(lw & 1u), b1 = __ballot(lw & 2u), b2 = __ballot(lw & 4u);
  if ((threadIdx.x & 63u) != 0u || !valid) return;
  const uint32_t g = r >> 6;
  if (FROM_Q) {
    a.live[(size_t)k * a.tw + 2 * g] = (uint32_t)bal;
    if (2 * g + 1 < a.tw) a.live[(size_t)k * a.tw + 2 * g + 1] = (uint32_t)(bal >> 32);
  }
  a.grp_rows[(size_t)k * a.groups + g] = (uint32_t)__popcll(bal);
  a.grp_cells[(size_t)k * a.groups + g] = cells_of(b0, b1, b2);
}

// one block per listed env: its groups' counts into exclusive prefixes and (totals) its totals into row_off /
// cell_off[k + 1]; a restore brings the offsets with it
__global__ void __launch_bounds__(SNAP_BLOCK) k_snap_scan_env(SnapArgs a, bool totals) {
  __shared__ uint32_t sr[SNAP_BLOCK], sc[SNAP_BLOCK];
  const uint32_t k = blockIdx.x, t = threadIdx.x;
  uint32_t* gr = a.grp_rows + (size_t)k * a.groups;
  uint32_t* gc = a.grp_cells + (size_t)k * a.groups;
  uint32_t carry_r = 0, carry_c = 0;
  for (uint32_t base = 0; base < a.groups; base += SNAP_BLOCK) {
    const uint32_t g = base + t;
    const uint32_t vr = g < a.groups ? gr[g] : 0u, vc = g < a.groups ? gc[g] : 0u;
    sr[t] = vr;
    sc[t] = vc;
    __syncthreads();
    for (uint32_t d = 1; d < SNAP_BLOCK; d <<= 1) {
      const uint32_t tr = t >= d ? sr[t - d] : 0u, tc = t >= d ? sc[t - d] : 0u;
      __syncthreads();
      sr[t] += tr;
      sc[t] += tc;
      __syncthreads();
    }
    if (g < a.groups) {
      gr[g] = carry_r + sr[t] - vr;
      gc[g] = carry_c + sc[t] - vc;
    }
    carry_r += sr[SNAP_BLOCK - 1];
    carry_c += sc[SNAP_BLOCK - 1];
    __syncthreads();
  }
  if (t == 0 && totals) {
    a.row_off[k + 1] = carry_r;
    a.cell_off[k + 1] = carry_c;
  }
}

// one block, any n: the envs' totals (at [k + 1]) into running offsets, 256 envs a round
__global__ void __launch_bounds__(SNAP_BLOCK) k_snap_scan_all(SnapArgs a) {
  __shared__ uint64_t sr[SNAP_BLOCK], sc[SNAP_BLOCK];
  const uint32_t t = threadIdx.x;
  uint64_t carry_r = 0, carry_c = 0;
  for (uint32_t base = 0; base < a.n; base += SNAP_BLOCK) {
    const uint32_t k = base + t;
    sr[t] = k < a.n ? a.row_off[k + 1] : 0ull;
    sc[t] = k < a.n ? a.cell_off[k + 1] : 0ull;
    __syncthreads();
    for (uint32_t d = 1; d < SNAP_BLOCK; d <<= 1) {
      const uint64_t tr = t >= d ? sr[t - d] : 0ull, tc = t >= d ? sc[t - d] : 0ull;
      __syncthreads();
      sr[t] += tr;
      sc[t] += tc;
      __syncthreads();
    }
    if (k < a.n) {
      a.row_off[k + 1] = carry_r + sr[t];
      a.cell_off[k + 1] = carry_c + sc[t];
    }
    carry_r += sr[SNAP_BLOCK - 1];
    carry_c += sc[SNAP_BLOCK - 1];
    __syncthreads();
  }
  if (t == 0) a.row_off[0] = a.cell_off[0] = 0ull;
}

// GATHER: a live row's id and cells into the packed buffers; else its cells from them into the env's block
template <bool GATHER>
__global__ void __launch_bounds__(SNAP_BLOCK) k_snap_rows(SnapArgs a, uint32_t rblocks) {
  const uint32_t k = blockIdx.x / rblocks;
  const uint32_t r = (blockIdx.x % rblocks) * SNAP_BLOCK + threadIdx.x;
  const size_t e = a.envs[k];
  const bool valid = r < a.rows;
  const uint32_t w = valid ? a.row_w[r] : 0u;
  const bool on = valid && ((a.live[(size_t)k * a.tw + (r >> 5)] >> (r & 31u)) & 1u);
  const uint32_t lw = on ? w : 0u;
  const uint64_t bal = __ballot(on), b0 = __ballot(lw & 1u), b1 = __ballot(lw & 2u), b2 = __ballot(lw & 4u);
  if (!on) return;
  const uint64_t below = (1ull << (threadIdx.x & 63u)) - 1ull;
  const size_t g = (size_t)k * a.groups + (r >> 6);
  const uint64_t ri = a.row_off[k] + a.grp_rows[g] + (uint32_t)__popcll(bal & below);
  const uint64_t ci = a.cell_off[k] + a.grp_cells[g] + cells_of(b0 & below, b1 & below, b2 & below);
  if (GATHER) a.row_ids[ri] = r;
  if (!w) return;
  uint64_t* p = a.q + e * a.Q + a.row_cell[r];
  for (uint32_t j = 0; j < w; ++j) {
    if (GATHER) a.cells[ci + j] = p[j];
    else p[j] = a.cells[ci + j];
  }
}

__global__ void __launch_bounds__(SNAP_BLOCK) k_snap_fill(SnapArgs a, uint32_t qblocks) {
  const uint32_t k = blockIdx.x / qblocks;
  const uint64_t i = (uint64_t)(blockIdx.x % qblocks) * SNAP_BLOCK + threadIdx.x;
  if (i < a.Q) a.q[(size_t)a.envs[k] * a.Q + i] = a.default_bits;
}

template <class T>
__device__ __forceinline__ void move(void* dev, void* rec, size_t di, size_t ri, bool gather) {
  if (gather) ((T*)rec)[ri] = ((const T*)dev)[di];
  else ((T*)dev)[di] = ((const T*)rec)[ri];
}

// one state array's slices of the listed envs <-> their place in the records.  Env-minor: neighbouring lanes take
// neighbouring list entries (coalesced on the array side when the list is a range); env-major: neighbouring elements
template <bool GATHER>
__global__ void __launch_bounds__(SNAP_BLOCK) k_snap_field(SnapField f, const uint32_t* envs, uint32_t n, uint32_t E,
                                                           uint8_t* state, uint32_t state_bytes) {
  const uint64_t t = (uint64_t)blockIdx.x * SNAP_BLOCK + threadIdx.x;
  if (t >= (uint64_t)n * f.count) return;
  const uint32_t k = f.major ? (uint32_t)(t / f.count) : (uint32_t)(t % n);
  const uint32_t i = f.major ? (uint32_t)(t % f.count) : (uint32_t)(t / n);
  const size_t e = envs[k];
  const size_t di = f.major ? e * f.count + i : (size_t)i * E + e;
  void* rec = state + (size_t)k * state_bytes + f.off;  // (f.off and state_bytes are multiples of f.elem)
  switch (f.elem) {
    case 1: move<uint8_t>(f.base, rec, di, i, GATHER); break;
    case 2: move<uint16_t>(f.base, rec, di, i, GATHER); break;
    case 4: move<uint32_t>(f.base, rec, di, i, GATHER); break;
    default: move<uint64_t>(f.base, rec, di, i, GATHER); break;
  }
}

}  // namespace

namespace sfl {

LaunchErr snap_launch(const SnapArgs& a, int phase, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (a.n == 0) return {};
  const uint64_t kMaxGrid = 0x7FFFFFFFull;
  const uint32_t rblocks = (a.rows + SNAP_BLOCK - 1) / SNAP_BLOCK;
  const uint32_t qblocks = (uint32_t)((a.Q + SNAP_BLOCK - 1) / SNAP_BLOCK);
  if ((uint64_t)a.n * rblocks > kMaxGrid || (uint64_t)a.n * qblocks > kMaxGrid)
    return launch_err("sfl_state: more than 2^31 blocks (envs x row tiles)", hipErrorInvalidConfiguration);
  const dim3 blk(SNAP_BLOCK);
  auto fields = [&](bool gather) -> hipError_t {
    SnapField keys{a.touched, 4u, a.tw, 1u, 0u};
    for (uint32_t f = 0; f <= a.n_fields; ++f) {
      const bool last = f == a.n_fields;
      const SnapField fd = last ? keys : a.fields[f];
      const uint64_t items = (uint64_t)a.n * fd.count;
      if (!items) continue;
      if ((items + SNAP_BLOCK - 1) / SNAP_BLOCK > kMaxGrid) return hipErrorInvalidConfiguration;
      const dim3 grid((uint32_t)((items + SNAP_BLOCK - 1) / SNAP_BLOCK));
      uint8_t* dst = last ? (uint8_t*)a.keys : a.state;
      const uint32_t stride = last ? a.tw * 4u : a.state_bytes;
      if (gather) hipLaunchKernelGGL(k_snap_field<true>, grid, blk, 0, stream, fd, a.envs, a.n, a.E, dst, stride);
      else hipLaunchKernelGGL(k_snap_field<false>, grid, blk, 0, stream, fd, a.envs, a.n, a.E, dst, stride);
    }
    return hipGetLastError();
  };
  if (phase == SNAP_COUNT) {
    if (rblocks) hipLaunchKernelGGL(k_snap_live<true>, dim3(a.n * rblocks), blk, 0, stream, a, rblocks);
    if (LaunchErr e = launch_err("k_snap_live")) return e;
    hipLaunchKernelGGL(k_snap_scan_env, dim3(a.n), blk, 0, stream, a, true);
    hipLaunchKernelGGL(k_snap_scan_all, dim3(1), blk, 0, stream, a);
    return launch_err("k_snap_scan");
  }
  if (phase == SNAP_GATHER) {
    if (rblocks) hipLaunchKernelGGL(k_snap_rows<true>, dim3(a.n * rblocks), blk, 0, stream, a, rblocks);
    if (LaunchErr e = launch_err("k_snap_rows")) return e;
    return launch_err("k_snap_field", fields(true));
  }
  if (qblocks) hipLaunchKernelGGL(k_snap_fill, dim3(a.n * qblocks), blk, 0, stream, a, qblocks);
  if (LaunchErr e = launch_err("k_snap_fill")) return e;
  if (rblocks) {
    hipLaunchKernelGGL(k_snap_live<false>, dim3(a.n * rblocks), blk, 0, stream, a, rblocks);
    hipLaunchKernelGGL(k_snap_scan_env, dim3(a.n), blk, 0, stream, a, false);
    hipLaunchKernelGGL(k_snap_rows<false>, dim3(a.n * rblocks), blk, 0, stream, a, rblocks);
  }
  if (LaunchErr e = launch_err("k_snap_rows")) return e;
  return launch_err("k_snap_field", fields(false));
}

}  // namespace sfl
