// Policy-bank evaluation, the traffic fold of a recording (include/sfl.h sfl_bank_record_traffic): the
// work description both backends take, the per-frame and per-row rule as functions both builds share, and the host
// build's plain loops.  Every output word is an integer sum over recorded frames or recorded decision rows, so the
// result does not depend on the order they are taken in: rec_traffic_host below, the kernels of sfl_rec.hip and the
// tests' numpy restatement agree exactly.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sfl.h"
#include "sfl_cells.h"
#include "sfl_launch.h"

namespace sfl {

enum : uint32_t { RC_S_MALF = 5 };  // the train state MALFUNCTION of a tr_bits word (sfl_core.h S_MALF), restated
enum { RC_DEC_WORDS = SFL_REC_DEC_WORDS, RC_SWITCH = 1, RC_ACTION = 6 };  // a decision row's words read here

struct RecArgs {
  uint32_t n, E, HW, S;        // recorded slots, envs, map cells, switches
  int32_t T, tick_cap, dec_cap;
  uint32_t p;                  // the policy whose slots are reduced
  const uint32_t* env;         // [n] slot -> env
  const uint32_t* policy;      // [E] the table each env followed in the last evaluation
  const int32_t* ticks;        // [E] the episode's true counts (the evaluation's outputs)
  const int32_t* dec;          // [E]
  const int32_t* cell;         // [n][tick_cap][T]
  const uint32_t* bits;        // [n][tick_cap][T]
  const int32_t* rows;         // [n][dec_cap][RC_DEC_WORDS]
  const uint8_t* sw_na;        // [S] actions of a switch: its STOP is action sw_na - 1 (SflMap)
  uint32_t* out;               // [3 * HW + 2 * S]: occupancy, standing, standing_malfunction, decisions, stops
};

// the kept frames / rows of slot k
SFL_CELL_FN int32_t rec_kept(int32_t count, int32_t cap) { return count < cap ? count : cap; }
// word w = (t - 1) * T + h of slot k's frames: what train h adds after tick t.  bit 0: occupancy of `c`, bit 1:
// standing, bit 2: standing in MALFUNCTION; 0 when the train is off the map (c = -1 then)
SFL_CELL_FN uint32_t rec_frame_word(const RecArgs& a, size_t base, size_t w, int32_t& c) {
  c = a.cell[base + w];
  if (c < 0 || (uint32_t)c >= a.HW) return 0u;
  uint32_t r = 1u;
  if (w >= (size_t)a.T && a.cell[base + w - (size_t)a.T] == c) {
    r |= 2u;
    if (((a.bits[base + w] >> 2) & 7u) == RC_S_MALF) r |= 4u;
  }
  return r;
}

// ---- the host build: plain loops ("device" memory is host memory here) ----------------------------------------------------
inline void rec_traffic_host(const RecArgs& a) {
  const size_t HW = a.HW;
  for (size_t i = 0; i < 3 * HW + 2 * (size_t)a.S; ++i) a.out[i] = 0u;
  for (uint32_t k = 0; k < a.n; ++k) {
    const uint32_t e = a.env[k];
    if (a.policy[e] != a.p) continue;
    const size_t base = (size_t)k * (size_t)a.tick_cap * (size_t)a.T;
    const size_t nw = (size_t)rec_kept(a.ticks[e], a.tick_cap) * (size_t)a.T;
    for (size_t w = 0; w < nw; ++w) {
      int32_t c;
      const uint32_t r = rec_frame_word(a, base, w, c);
      if (r & 1u) a.out[c] += 1u;
      if (r & 2u) a.out[HW + c] += 1u;
      if (r & 4u) a.out[2 * HW + c] += 1u;
    }
    const int32_t* rows = a.rows + (size_t)k * (size_t)a.dec_cap * RC_DEC_WORDS;
    const int32_t nd = rec_kept(a.dec[e], a.dec_cap);
    for (int32_t d = 0; d < nd; ++d) {
      const uint32_t sw = (uint32_t)rows[(size_t)d * RC_DEC_WORDS + RC_SWITCH];
      if (sw >= a.S) continue;
      a.out[3 * HW + sw] += 1u;
      if (rows[(size_t)d * RC_DEC_WORDS + RC_ACTION] == (int32_t)a.sw_na[sw] - 1) a.out[3 * HW + a.S + sw] += 1u;
    }
  }
}

// sfl_rec.hip: queues the kernel that empties `out` and k_rec_traffic on `stream` (a hipStream_t); the failing launch,
// if any (sfl_launch.h)
LaunchErr rec_traffic_launch(const RecArgs& a, void* stream);

}  // namespace sfl
