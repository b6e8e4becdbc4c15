// Suspend and resume (include/sfl.h sfl_state_*): the work description both backends take, and the
// host build's plain loops.  A capture of n listed envs is their small per-env state (one record of state_bytes per
// env), their key sets, and only the Q rows that hold something:
//   row r of env e is LIVE when its key-set bit is set or any of its cells differs from default_q as a 64-bit pattern;
//   row_ids[row_off[k] .. row_off[k + 1]) are the live rows of the k-th listed env in ascending order, and
//   cells[cell_off[k] .. cell_off[k + 1]) their cells as bit patterns, rows in row_ids order, a row's cells in stored order.
// snap_host below and the kernels of sfl_snap.hip are two implementations that agree byte for byte.
#pragma once
#include <stdint.h>
#include <string.h>

#include "sfl_launch.h"

namespace sfl {

// One SflState array as the capture sees it: `count` elements of `elem` bytes per env, env-minor (element i of env e at
// index i * E + e: the lane-per-env body's arrays, and every per-env scalar) or env-major (at e * count + i: the wave
// kernels' per-train, per-port and per-switch arrays between launches); `off`: its place in the env's record
struct SnapField {
  void* base;
  uint32_t elem, count, major, off;
};
constexpr int SNAP_MAX_FIELDS = 40;
constexpr uint32_t SNAP_GROUP = 64;  // rows per scan group: a wavefront's ballot

enum : int { SNAP_COUNT = 0, SNAP_GATHER = 1, SNAP_RESTORE = 2 };
enum : uint32_t { SNAP_LANE = 0, SNAP_WAVE = 1 };  // layout class of a record (sfl_state_info.layout)

struct SnapArgs {
  uint32_t E, n, tw, rows, groups;  // groups: scan groups per env, ceil(rows / SNAP_GROUP)
  uint32_t state_bytes, n_fields;
  uint64_t Q, default_bits;
  uint64_t* q;               // [E][Q] as bit patterns
  uint32_t* touched;         // [E][tw]
  const uint64_t* row_cell;  // [rows] offset of the row's first cell in an env's block
  const uint8_t* row_w;      // [rows] cells of the row (0: a row id of no block)
  const uint32_t* envs;      // [n] the listed envs (capture) or slots (restore)
  uint32_t* live;            // [n][tw] live-row bitmap (capture: scratch; restore: from the record's row ids)
  uint32_t* grp_rows;        // [n][groups] live rows in the env's groups before this one (SNAP_COUNT leaves the prefix)
  uint32_t* grp_cells;       // [n][groups] their cells
  uint64_t* row_off;         // [n + 1]
  uint64_t* cell_off;        // [n + 1]
  uint32_t* row_ids;         // [row_off[n]]
  uint64_t* cells;           // [cell_off[n]]
  uint32_t* keys;            // [n][tw] the listed envs' key sets
  uint8_t* state;            // [n][state_bytes]
  SnapField fields[SNAP_MAX_FIELDS];
};

inline void snap_copy(void* d, const void* s, uint32_t elem) { memcpy(d, s, elem); }
// (the host build's Q block is written as doubles elsewhere in the same translation unit: no access through a uint64_t lvalue)
inline uint64_t snap_ld(const uint64_t* p) {
  uint64_t v;
  memcpy(&v, p, 8);
  return v;
}
inline void snap_st(uint64_t* p, uint64_t v) { memcpy(p, &v, 8); }

// the host build: the rule as written, one env at a time ("device" memory is host memory here)
inline void snap_host(const SnapArgs& a, int phase) {
  for (uint32_t k = 0; k < a.n; ++k) {
    const size_t e = a.envs[k];
    uint64_t* q = a.q + e * a.Q;
    uint32_t* keys = a.touched + e * a.tw;
    uint32_t* live = a.live + (size_t)k * a.tw;
    if (phase == SNAP_COUNT) {
      uint64_t nr = 0, nc = 0;
      for (uint32_t w = 0; w < a.tw; ++w) live[w] = 0;
      for (uint32_t r = 0; r < a.rows; ++r) {
        bool on = (keys[r >> 5] >> (r & 31u)) & 1u;
        for (uint32_t j = 0; j < a.row_w[r]; ++j) on = on || snap_ld(q + a.row_cell[r] + j) != a.default_bits;
        if (!on) continue;
        live[r >> 5] |= 1u << (r & 31u);
        ++nr;
        nc += a.row_w[r];
      }
      if (k == 0) a.row_off[0] = a.cell_off[0] = 0;
      a.row_off[k + 1] = a.row_off[k] + nr;
      a.cell_off[k + 1] = a.cell_off[k] + nc;
      continue;
    }
    const bool out = phase == SNAP_GATHER;
    if (!out)
      for (uint64_t i = 0; i < a.Q; ++i) snap_st(q + i, a.default_bits);
    uint64_t ri = a.row_off[k], ci = a.cell_off[k];
    for (uint32_t r = 0; r < a.rows; ++r) {
      if (!((live[r >> 5] >> (r & 31u)) & 1u)) continue;
      if (out) a.row_ids[ri] = r;
      ++ri;
      for (uint32_t j = 0; j < a.row_w[r]; ++j, ++ci) {
        if (out) a.cells[ci] = snap_ld(q + a.row_cell[r] + j);
        else snap_st(q + a.row_cell[r] + j, a.cells[ci]);
      }
    }
    for (uint32_t w = 0; w < a.tw; ++w) {
      if (out) a.keys[(size_t)k * a.tw + w] = keys[w];
      else keys[w] = a.keys[(size_t)k * a.tw + w];
    }
    for (uint32_t f = 0; f < a.n_fields; ++f) {
      const SnapField& fd = a.fields[f];
      for (uint32_t i = 0; i < fd.count; ++i) {
        char* dev = (char*)fd.base + (fd.major ? e * fd.count + i : (size_t)i * a.E + e) * fd.elem;
        char* rec = (char*)a.state + (size_t)k * a.state_bytes + fd.off + (size_t)i * fd.elem;
        if (out) snap_copy(rec, dev, fd.elem);
        else snap_copy(dev, rec, fd.elem);
      }
    }
  }
}

// sfl_snap.hip: queues the kernels of one phase on `stream` (a hipStream_t); the failing launch, if any
// (sfl_launch.h)
LaunchErr snap_launch(const SnapArgs& a, int phase, void* stream);

}  // namespace sfl
