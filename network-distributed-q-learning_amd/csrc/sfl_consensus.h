// Consensus Q-tables (include/sfl.h sfl_consensus): the work description both backends take, and the host build's
// plain loops.  The merge rule is stated once, in DESIGN.md "Consensus Q-tables"; consensus_host below, the kernels
// of sfl_consensus.hip and the test model (tests/_consensus.py) are three implementations of it that agree bit for bit.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/sfl.h"
#include "sfl_launch.h"

namespace sfl {

constexpr uint32_t CONS_NO_ROW = 0xFFFFFFFFu;  // cell_row: a cell of no block (never held)
constexpr uint32_t CONS_DIRECT = 0xFFFFFFFFu;  // ConsJob::slot: the job is its cohort's only chunk and writes the table

// One chunk of a cohort's member list: members[begin .. begin + n) (n <= SFL_CONSENSUS_CHUNK, ascending env index).
// A cohort of at most one chunk (an empty one too) has one job with slot == CONS_DIRECT; a longer one has a job per
// chunk, slot = the chunk's partial record, and a ConsCombo that combines the slots [slot0, slot0 + n_chunks) in order.
struct ConsJob {
  uint32_t begin, n, cohort, slot;
};
struct ConsCombo {
  uint32_t slot0, n_chunks, cohort, pad_;
};

// meta word of a partial record: contributor count (<= 256) | all-equal << 16 | some holder << 17
constexpr uint32_t CONS_M_EQ = 1u << 16, CONS_M_HELD = 1u << 17, CONS_M_COUNT = 0xFFFFu;

struct ConsArgs {
  int32_t mode;
  uint32_t flags;
  uint32_t E, n_cohorts, tw;  // tw: key-set words per env
  uint32_t n_jobs, n_combos, n_slots;
  uint64_t Q;          // cells per env
  uint64_t cells_cap;  // cells of a partial-record slot: q_per_env rounded up to the kernels' tile (the scratch holds
                       // n_slots * cells_cap records)
  uint64_t default_bits;
  double* q;                  // [E][Q]
  uint32_t* touched;          // [E][tw]
  const uint32_t* cell_row;   // [Q] row id of each cell (k_qinit's row_base + state), CONS_NO_ROW for none
  const uint32_t* members;    // member envs, grouped by cohort in cohort order, ascending env index inside one
  const uint32_t* coh_off;    // [n_cohorts + 1] offsets into members
  const ConsJob* jobs;        // [n_jobs]
  const ConsCombo* combos;    // [n_combos]
  double* cons_q;             // [n_cohorts][Q]
  uint32_t* cons_keys;        // [n_cohorts][tw]
  // partial records of the chunks of cohorts longer than one chunk (HIP backend only)
  double* p_sum;              // [n_slots][cells_cap]
  uint64_t* p_first;          // [n_slots][cells_cap]
  uint32_t* p_meta;           // [n_slots][cells_cap]
  uint32_t* p_keys;           // [n_slots][tw]
};

inline uint64_t cons_bits(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}
inline double cons_f64(uint64_t b) {
  double v;
  memcpy(&v, &b, 8);
  return v;
}

// The host build: the rule as written, one cohort, one cell at a time ("device" memory is host memory here).
inline void consensus_host(const ConsArgs& a) {
  const double dq = cons_f64(a.default_bits);
  for (uint32_t c = 0; c < a.n_cohorts; ++c) {
    const uint32_t* mem = a.members + a.coh_off[c];
    const uint32_t n = a.coh_off[c + 1] - a.coh_off[c];
    uint32_t* keys = a.cons_keys + (size_t)c * a.tw;
    for (uint32_t w = 0; w < a.tw; ++w) {
      uint32_t k = 0;
      for (uint32_t j = 0; j < n; ++j) k |= a.touched[(size_t)mem[j] * a.tw + w];
      keys[w] = k;
    }
    double* out = a.cons_q + (size_t)c * a.Q;
#ifdef _OPENMP
#pragma omp parallel for
#endif
    for (int64_t i = 0; i < (int64_t)a.Q; ++i) {
      const uint32_t r = a.cell_row[i];
      auto holds = [&](uint32_t e) {
        return r != CONS_NO_ROW && ((a.touched[(size_t)e * a.tw + (r >> 5)] >> (r & 31u)) & 1u) != 0u;
      };
      double res = dq;
      if (a.mode == SFL_CONSENSUS_MAX) {
        bool have = false;
        for (uint32_t j = 0; j < n; ++j) {
          if (!holds(mem[j])) continue;
          const double v = a.q[(size_t)mem[j] * a.Q + i];
          if (!have || v > res) res = v;
          have = true;
        }
      } else {
        uint64_t first = 0, count = 0;
        bool eq = true;
        double total = 0.0;
        for (uint32_t j0 = 0; j0 < n; j0 += SFL_CONSENSUS_CHUNK) {
          double part = 0.0;
          for (uint32_t j = j0; j < n && j < j0 + SFL_CONSENSUS_CHUNK; ++j) {
            if (!holds(mem[j])) continue;
            const double v = a.q[(size_t)mem[j] * a.Q + i];
            const uint64_t b = cons_bits(v);
            if (b == a.default_bits) continue;
            if (count == 0) first = b;
            else if (b != first) eq = false;
            ++count;
            part = part + v;
          }
          total = total + part;
        }
        if (count) res = eq ? cons_f64(first) : total / (double)count;
      }
      out[i] = res;
    }
    if (!(a.flags & SFL_CONSENSUS_SHARE)) continue;
    for (uint32_t j = 0; j < n; ++j) {
      double* q = a.q + (size_t)mem[j] * a.Q;
      for (uint64_t i = 0; i < a.Q; ++i) {
        const uint32_t r = a.cell_row[i];
        if (r != CONS_NO_ROW && ((keys[r >> 5] >> (r & 31u)) & 1u)) q[i] = out[i];
      }
      for (uint32_t w = 0; w < a.tw; ++w) a.touched[(size_t)mem[j] * a.tw + w] |= keys[w];
    }
  }
}

// sfl_consensus.hip: queues the kernels of one call on `stream` (a hipStream_t); the failing launch, if any
// (sfl_launch.h)
LaunchErr consensus_launch(const ConsArgs& a, void* stream);
constexpr uint32_t CONS_TILE = 512;  // cells per block of the kernels (cells_cap is a multiple of it)

}  // namespace sfl
