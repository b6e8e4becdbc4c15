// External-action mode's transition assembler (include/sfl.h sfl_env_trans_*): the learner's pending
// table (distr_q.py:283, 322-356; env_post in sfl_core.h) kept behind the env step, so that a policy on the device
// gets complete transitions (agent, obs, action, reward, next_agent, next_obs, next_action_mask, terminal) in a
// replay ring in device memory.  The per-env logic, the row encode and the host build's loops are here, written once
// for host and device; the kernels are in sfl_trans.hip.  Both produce the same bytes.
//
// Per env e, with (s, h, slot, state, mask, r, now) the decision the PREVIOUS call emitted (latched by the assembler:
// the step overwrites the caller's buffers) and a the action a call applied to it (a >= 0, next_switch >= 0):
//   1. an entry at (s, h) gives the row {its agent, obs, action; reward r; next = (s, obs, mask); terminal 0} and goes;
//   2. table[(next_switch, h)] = (s, slot, state, a, now)   (an entry already there is overwritten);
//   3. for each train of arrived & ~seen in ascending order, each entry of that train in ascending switch order gives
//      the row {its agent, obs, action; reward DEST_BONUS; next_agent -1, next_obs -1, mask 0; terminal 1} and goes;
//      seen |= arrived;
//   4. at an episode end (agent == -1) or SFL_ACTION_RESET: dropped[e] += live entries, the table empties, seen = 0
//      (after 1-3 at an episode end; alone at a reset).
// Rows of a call are ranked env by env (in the order above within an env); row r of the call is row total + r of
// the run and lands in ring slot (total + r) % N; of a call with more than N rows only the last N are written.
//
// The table is [E][T][S] entries of 16 bytes, a train's S entries contiguous (step 3 reads them as one run).  An entry
// is live while its stamp equals its env's episode count + 1; step 4 advances the count (32 bits: it does not wrap
// before 2^32 - 1 episodes of one env), so nothing is cleared by writing.
#pragma once
#include <stdint.h>

#include "sfl_core.h"
#include "sfl_launch.h"

namespace sfl {

constexpr int32_t DEST_BONUS = 1000;  // SFL_DEST_BONUS: env_post's destination bonus (distr_q.py destination_bonus)
constexpr int TRANS_BLOCK = 256;      // envs per block of the kernels: the unit of the cross-block prefix

struct alignas(16) TransEntry {
  uint32_t who;    // agent | slot << 16 | action << 24
  uint32_t state;  // observation index
  int32_t now;     // elapsed ticks at the decision
  uint32_t stamp;  // live: the env's episode count + 1
};
struct alignas(16) TransLatch {  // the decision a call emitted (agent -1: none)
  int32_t agent, train, slot;
  uint32_t state, mask;
  int32_t reward, now, pad_;
};

struct TransArgs {
  uint32_t E, N;  // envs; ring capacity
  int32_t S, T, K;
  uint32_t parity;  // which of the two cursors this call reads (it writes the other)
  // what the env step of this call read and wrote (SflExt)
  const int32_t* actions;
  const int32_t* agent;
  const int32_t* train;
  const int32_t* slot;
  const uint32_t* state;
  const uint32_t* mask;
  const int32_t* reward;
  const int32_t* now;
  const int32_t* next_sw;
  const uint32_t* arrived;  // [MAXW][E]
  // the observation decode's tables (SflEnc)
  const uint8_t* sw_np;
  const uint8_t* sw_na;
  const int32_t* sw_rc;
  const int32_t* st_rc;
  // the assembler's own state
  TransEntry* tab;    // [E][T][S]
  TransLatch* latch;  // [E]
  uint32_t* live;     // [E] live entries
  uint32_t* seen;     // [MAXW][E] arrived trains already credited
  uint32_t* epoch;    // [E] episodes ended (or reset) since sfl_env_trans_begin
  uint32_t* cnt;      // [E] rows of this call (counting pass -> writing pass)
  uint32_t* blk;      // [ceil(E / TRANS_BLOCK)] their sums per block of envs
  uint64_t* cur;      // [2][2] (total, total % N): read at [parity], written at [1 - parity]
  // the ring's columns ([N]; obs / next_obs [N][OBS_WIDTH], next_mask [N][MAX_ACTIONS]: null skips one of the three)
  int32_t *r_env, *r_train, *r_now, *r_agent, *r_action, *r_reward, *r_next_agent, *r_next_na;
  uint8_t* r_terminal;
  int32_t *r_obs, *r_next_obs;
  uint8_t* r_next_mask;
  int64_t* total;       // [1] rows emitted since begin
  int32_t* last_count;  // [1] rows of the last call
  int64_t* dropped;     // [E] entries dropped at episode ends and resets
};

// an env's part of a call that takes one lane: everything but the entries of newly arrived trains
struct TransEnv {
  TransLatch p;      // the previous call's decision
  int32_t act, nsw;  // this call's action and its successor switch
  uint32_t epoch, live;
  uint32_t fresh[MAXW];
  TransEntry got;    // the entry step 1 takes
  bool applied, consumed, next_old, any_fresh, clear;
};

// one ring row before its decode
struct TransRow {
  uint32_t slot;
  int32_t env, train, now, agent, pslot;
  uint32_t pstate;
  int32_t action, reward, nagent, nslot;
  uint32_t nstate, nmask;
};

SFL_FN bool trans_bit(const uint32_t (&f)[MAXW], int t) {  // (no indexed access: the words stay in registers)
  uint32_t w = 0u;
#pragma unroll
  for (int i = 0; i < MAXW; ++i) w = (t >> 5) == i ? f[i] : w;
  return (w >> (t & 31)) & 1u;
}
SFL_FN size_t trans_ix(const TransArgs& a, uint32_t e, int h, int sw) { return ((size_t)e * a.T + h) * a.S + sw; }

SFL_FN void trans_env_head(const TransArgs& a, uint32_t e, TransEnv& v) {
  v.p = a.latch[e];
  v.act = a.actions[e];
  v.nsw = a.next_sw[e];
  v.epoch = a.epoch[e];
  v.live = a.live[e];
  v.applied = v.act >= 0 && v.nsw >= 0 && v.p.agent >= 0;
  v.clear = a.agent[e] < 0 || v.act == -2;  // the episode ended in this call, or SFL_ACTION_RESET
  v.consumed = v.next_old = v.any_fresh = false;
#pragma unroll
  for (int w = 0; w < MAXW; ++w) v.fresh[w] = 0u;
  v.got = TransEntry{0u, 0u, 0, 0u};
  if (!v.applied) return;
  v.got = a.tab[trans_ix(a, e, v.p.train, v.p.agent)];
  v.consumed = v.got.stamp == v.epoch + 1u;
  // was (next_switch, h) live before step 2 (after step 1 took (s, h))?
  v.next_old = v.nsw != v.p.agent && a.tab[trans_ix(a, e, v.p.train, v.nsw)].stamp == v.epoch + 1u;
#pragma unroll
  for (int w = 0; w < MAXW; ++w) {
    const int left = a.T - 32 * w;  // (trains of this word: no bit past T is ever walked)
    const uint32_t trains = left >= 32 ? 0xFFFFFFFFu : left <= 0 ? 0u : (1u << left) - 1u;
    v.fresh[w] = a.arrived[(size_t)w * a.E + e] & ~a.seen[(size_t)w * a.E + e] & trains;
    v.any_fresh = v.any_fresh || v.fresh[w] != 0u;
  }
}

// what step 3 needs of the env whose train it walks (one wavefront walks it together: the values are broadcast)
struct TransScan {
  uint32_t e, epoch;
  int32_t h, s, nsw;    // the deciding train, its switch, the successor switch
  TransEntry made;      // the entry step 2 writes at (nsw, h)
};
SFL_FN TransEntry trans_made(const TransEnv& v) {
  return TransEntry{(uint32_t)v.p.agent | (uint32_t)v.p.slot << 16 | (uint32_t)v.act << 24, v.p.state, v.p.now, v.epoch + 1u};
}
// entry (sw, tr) as step 3 finds it, after steps 1 and 2 (which are written after the walk): live or not, and its content
SFL_FN bool trans_live(const TransScan& c, int tr, int sw, TransEntry& x) {
  if (tr == c.h) {
    if (sw == c.nsw) {
      x = c.made;
      return true;
    }
    if (sw == c.s) return false;
  }
  return x.stamp == c.epoch + 1u;
}

SFL_FN TransRow trans_row_next(const TransEnv& v, uint32_t e) {  // step 1's row
  TransRow r;
  r.slot = 0u;
  r.env = (int32_t)e;
  r.train = v.p.train;
  r.now = v.got.now;
  r.agent = (int32_t)(v.got.who & 0xFFFFu);
  r.pslot = (int32_t)((v.got.who >> 16) & 0xFFu);
  r.pstate = v.got.state;
  r.action = (int32_t)(v.got.who >> 24);
  r.reward = v.p.reward;
  r.nagent = v.p.agent;
  r.nslot = v.p.slot;
  r.nstate = v.p.state;
  r.nmask = v.p.mask;
  return r;
}
SFL_FN TransRow trans_row_bonus(const TransEntry& x, uint32_t e, int tr) {  // one of step 3's rows
  TransRow r;
  r.slot = 0u;
  r.env = (int32_t)e;
  r.train = tr;
  r.now = x.now;
  r.agent = (int32_t)(x.who & 0xFFFFu);
  r.pslot = (int32_t)((x.who >> 16) & 0xFFu);
  r.pstate = x.state;
  r.action = (int32_t)(x.who >> 24);
  r.reward = DEST_BONUS;
  r.nagent = -1;
  r.nslot = 0;
  r.nstate = 0u;
  r.nmask = 0u;
  return r;
}

// ring slot of the call's row `rank`; head = total % N before the call, over: the call has more rows than the ring
SFL_FN uint32_t trans_slot(uint64_t head, uint64_t rank, uint32_t N, bool over) {
  const uint64_t x = head + rank;
  if (!over) return (uint32_t)(x >= N ? x - N : x);  // (rank < N)
  return (uint32_t)(x % N);
}

// pair p of a row's obs (p < OBS_PAIRS) or next_obs (p - OBS_PAIRS): obs_pair on the words the row carries
SFL_FN void trans_store_pair(const TransArgs& a, const TransRow& r, uint32_t p) {
  const bool nxt = p >= (uint32_t)OBS_PAIRS;
  int32_t* dst = nxt ? a.r_next_obs : a.r_obs;
  if (!dst) return;
  const int32_t ag = nxt ? r.nagent : r.agent, sl = nxt ? r.nslot : r.pslot;
  const uint32_t st = nxt ? r.nstate : r.pstate;
  SflEnc x{};
  x.K = a.K;
  x.agent = &ag;
  x.slot = &sl;
  x.state = &st;
  x.sw_np = a.sw_np;
  x.sw_rc = a.sw_rc;
  x.st_rc = a.st_rc;
  const uint32_t q = nxt ? p - (uint32_t)OBS_PAIRS : p;
  *(ObsPair*)(dst + (size_t)OBS_WIDTH * r.slot + 2 * q) = obs_pair(x, 0u, q);
}

// a row's scalar columns and its mask row (env_encode_item's packing: byte a = bit a of the mask, one 16-byte store)
SFL_FN void trans_store_scalars(const TransArgs& a, const TransRow& r) {
  const size_t i = r.slot;
  a.r_env[i] = r.env;
  a.r_train[i] = r.train;
  a.r_now[i] = r.now;
  a.r_agent[i] = r.agent;
  a.r_action[i] = r.action;
  a.r_reward[i] = r.reward;
  a.r_next_agent[i] = r.nagent;
  const uint32_t na = r.nagent < 0 ? 0u : a.sw_na[r.nagent];
  a.r_next_na[i] = (int32_t)na;
  a.r_terminal[i] = r.nagent < 0 ? 1 : 0;
  if (a.r_next_mask) {
    const uint32_t m = r.nagent < 0 ? 0u : r.nmask & ((1u << na) - 1u);
    MaskRow w{0, 0};
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      w.lo |= (uint64_t)((m >> b) & 1u) << (8 * b);
      w.hi |= (uint64_t)((m >> (8 + b)) & 1u) << (8 * b);
    }
    *(MaskRow*)(a.r_next_mask + (size_t)MAX_ACTIONS * i) = w;
  }
}
SFL_FN void trans_store_row(const TransArgs& a, const TransRow& r) {
  trans_store_scalars(a, r);
  for (uint32_t p = 0; p < 2u * OBS_PAIRS; ++p) trans_store_pair(a, r, p);
}

// the env's own writes, after its rows are out: steps 1 and 2 on the table (entries step 3 took are cleared by the walk),
// the live count, seen, step 4, and the decision this call emitted for the next one.  n: the env's rows of this call
SFL_FN void trans_env_tail(const TransArgs& a, uint32_t e, TransEnv& v, uint32_t n) {
  if (v.applied) {
    const bool h_fresh = trans_bit(v.fresh, v.p.train);
    v.live = v.live - n + (v.next_old ? 0u : 1u);
    if (v.consumed && v.nsw != v.p.agent) a.tab[trans_ix(a, e, v.p.train, v.p.agent)].stamp = 0u;
    if (!h_fresh) a.tab[trans_ix(a, e, v.p.train, v.nsw)] = trans_made(v);
    if (v.any_fresh && !v.clear) {
#pragma unroll
      for (int w = 0; w < MAXW; ++w) a.seen[(size_t)w * a.E + e] |= v.fresh[w];
    }
  }
  if (v.clear) {
    a.dropped[e] += (int64_t)v.live;
    v.live = 0u;
    v.epoch += 1u;
#pragma unroll
    for (int w = 0; w < MAXW; ++w) a.seen[(size_t)w * a.E + e] = 0u;
  }
  a.live[e] = v.live;
  a.epoch[e] = v.epoch;
  TransLatch l;
  l.agent = a.agent[e];
  l.train = a.train[e];
  l.slot = a.slot[e];
  l.state = a.state[e];
  l.mask = a.mask[e];
  l.reward = a.reward[e];
  l.now = a.now[e];
  l.pad_ = 0;
  a.latch[e] = l;
}

SFL_FN TransScan trans_scan_of(const TransEnv& v, uint32_t e) {
  TransScan c;
  c.e = e;
  c.epoch = v.epoch;
  c.h = v.p.train;
  c.s = v.p.agent;
  c.nsw = v.nsw;
  c.made = trans_made(v);
  return c;
}

// the host build: the same two passes as plain loops ("device" memory is host memory here)
inline void trans_host(const TransArgs& a) {
  // counting pass
  uint64_t C = 0;
  for (uint32_t e = 0; e < a.E; ++e) {
    TransEnv v;
    trans_env_head(a, e, v);
    uint32_t n = v.consumed ? 1u : 0u;
    if (v.any_fresh) {
      const TransScan c = trans_scan_of(v, e);
      for (int tr = 0; tr < a.T; ++tr) {
        if (!trans_bit(v.fresh, tr)) continue;
        for (int sw = 0; sw < a.S; ++sw) {
          TransEntry x = a.tab[trans_ix(a, e, tr, sw)];
          n += trans_live(c, tr, sw, x) ? 1u : 0u;
        }
      }
    }
    a.cnt[e] = n;
    C += n;
  }
  // writing pass
  const uint64_t total = a.cur[2 * a.parity], head = a.cur[2 * a.parity + 1];
  const bool over = C > a.N;
  const uint64_t skip = over ? C - a.N : 0u;
  uint64_t rank = 0;
  for (uint32_t e = 0; e < a.E; ++e) {
    TransEnv v;
    trans_env_head(a, e, v);
    if (v.consumed) {
      if (rank >= skip) {
        TransRow r = trans_row_next(v, e);
        r.slot = trans_slot(head, rank, a.N, over);
        trans_store_row(a, r);
      }
      ++rank;
    }
    if (v.any_fresh) {
      const TransScan c = trans_scan_of(v, e);
      for (int tr = 0; tr < a.T; ++tr) {
        if (!trans_bit(v.fresh, tr)) continue;
        for (int sw = 0; sw < a.S; ++sw) {
          TransEntry x = a.tab[trans_ix(a, e, tr, sw)];
          if (!trans_live(c, tr, sw, x)) continue;
          if (rank >= skip) {
            TransRow r = trans_row_bonus(x, e, tr);
            r.slot = trans_slot(head, rank, a.N, over);
            trans_store_row(a, r);
          }
          ++rank;
          a.tab[trans_ix(a, e, tr, sw)].stamp = 0u;
        }
      }
    }
    trans_env_tail(a, e, v, a.cnt[e]);
  }
  uint64_t* nxt = a.cur + 2 * (1u - a.parity);
  nxt[0] = total + C;
  nxt[1] = (head + C) % a.N;
  *a.total = (int64_t)(total + C);
  *a.last_count = (int32_t)C;
}

// sfl_trans.hip: queues the two kernels on `stream` (a hipStream_t); the failing launch, if any (sfl_launch.h)
LaunchErr trans_launch(const TransArgs& a, void* stream);

}  // namespace sfl
