// Engine: owns one batch of lock-step environments on one device and implements
// the C-ABI of include/sfl.h.  Templated over a backend (HIP device memory +
// kernel launches in sfl.hip; host memory + a plain loop in the test-only
// host build sfl_hostsim.cpp) so both builds share every line above the
// per-env kernel body.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sfl.h"
#include "sfl_consensus.h"
#include "sfl_core.h"
#include "sfl_curve.h"
#include "sfl_diag.h"
#include "sfl_eval.h"
#include "sfl_mfgen.h"
#include "sfl_part.h"
#include "sfl_rec.h"
#include "sfl_snap.h"
#include "sfl_trans.h"

namespace sfl {

static thread_local std::string g_last_error;

inline int fail(const std::string& msg) {
  g_last_error = msg;
  return -1;
}

// FNV-1a over bytes: the fingerprints of sfl_state_info (a state record names cells, rows, ports and trains of its map)
inline uint64_t snap_hash(uint64_t h, const void* p, size_t n) {
  const uint8_t* b = (const uint8_t*)p;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
  return h;
}
inline uint64_t snap_map_fp(const sfl_map_desc* md) {
  uint64_t h = 0xCBF29CE484222325ull;
  const size_t HW = (size_t)md->H * md->W, NP = (size_t)md->S * 4, S = md->S, T = md->T;
  const int64_t sc[] = {md->H, md->W, md->S, md->T, md->K, md->max_episode_steps, md->mf_min, md->mf_max,
                        (int64_t)md->q_per_env, (int64_t)md->rows_per_env};
  h = snap_hash(h, sc, sizeof sc);
  h = snap_hash(h, &md->mf_rate, 8);
  auto arr = [&](const void* p, size_t bytes) { h = snap_hash(snap_hash(h, &bytes, sizeof bytes), p, bytes); };
  arr(md->grid, HW * 2);
  arr(md->cell_sw, HW * 2);
  arr(md->sw_np, S);
  arr(md->sw_na, S);
  arr(md->act_src, S * 8);
  arr(md->act_dst, S * 8);
  arr(md->act_turn, S * 8);
  arr(md->act_j, S * 8);
  arr(md->first_other, NP);
  arr(md->port_side, NP);
  arr(md->slot_nroutes, NP);
  arr(md->slot_route_act, NP * 4);
  arr(md->q_w, NP);
  arr(md->port_nb, NP * 2);
  arr(md->port_len, NP * 2);
  arr(md->port_unique, NP * 2);
  arr(md->q_off, NP * 8);
  arr(md->row_base, NP * 4);
  arr(md->dist, (size_t)md->K * HW * 4 * 4);
  for (const int32_t* p : {md->tr_ed, md->tr_la, md->tr_k, md->tr_target, md->tr_init_cell, md->tr_init_dist, md->tr_init_delay})
    arr(p, T * 4);
  arr(md->tr_init_dir, T);
  arr(md->tr_init_port, T * 2);
  return h;
}

template <class B>
struct Handle {
  B be;
  SflMap map{};
  SflState st{};
  uint32_t E = 0;
  int device = 0;
  std::vector<void*> allocs;
  std::vector<uint64_t> seeds;
  // host copies of small per-env counters for reporting
  // launch totals reduced on the device (decisions, ticks, algorithmic bytes, OR of error flags)
  uint64_t last_dec = 0, last_ticks = 0, last_bytes = 0, total_dec = 0;
  uint32_t last_err = 0;
  uint64_t* d_sums = nullptr;  // [4]
  bool ext_stream = false;     // the caller's stream (sfl_set_stream): owner steps queue without a sync
  bool part_pending = false;              // a part_local's counts not read yet
  bool part_consumed = true;              // part_counts handed out by sfl_part_counts (the next read restarts the peaks)
  uint64_t part_reads = 0;                // host reads of the round counts (part_read): sfl_get_sync_count
  std::vector<uint32_t> part_counts;      // of the last part_local: [2 * world + 1]
  // the partitioned wave kernels' per-env scalar blocks (SflPart::eblk): which copy is current --
  // 0 the SflState arrays (the next part_local copies them in), 1 the blocks, 2 both
  int eblk_state = 0;
  uint64_t* d_launch_dec = nullptr;
  uint64_t* d_launch_ticks = nullptr;
  uint64_t* d_launch_bytes = nullptr;
  float last_kernel_ms = 0.f;
  std::vector<std::vector<uint32_t>> keep;  // host sources of async uploads, alive until the create() sync
  int variant = 0;  // 0: k_run (lane per env); v > 0: k_wave shape kVariants[v] (see choose_variant)
  int created_variant = 0;  // choose_variant's row at create: sfl_env_begin puts the handle on the lane-per-env body
                            // (variant = 0), sfl_env_begin_wave back on this row (ext_variant)
  std::string variant_note;  // why a device handle runs k_run ("" when k_wave, or when chosen explicitly)
  // host copies of the map fields the partitioned mode lays out its owned Q blocks with
  std::vector<uint8_t> h_sw_np, h_q_w;
  std::vector<uint64_t> h_q_off;
  std::vector<uint32_t> h_row_base;
  // graph-partitioned mode (sfl_part.h); part.world == 0: not configured
  SflPart part{};
  // external-action mode (sfl_env_begin / sfl_env_step): device buffers, the descriptor in device memory
  SflExt ext{};
  SflExt* d_ext = nullptr;
  bool env_mode = false;
  // the observation decode's coordinate tables (sfl_env_step_dev), derived at create: switch cells from cell_sw,
  // station cells from tr_k / tr_target; max_na: the widest action space (the dense mask holds SFL_MAX_ACTIONS)
  int32_t* d_sw_rc = nullptr;  // [S][2]
  int32_t* d_st_rc = nullptr;  // [K][2]
  int max_na = 0;
  // per-phase cycles of the sampled wavefronts, accumulated over learn / test launches on the device
  // (sfl_get_phase_cycles reads them)
  uint64_t* d_phase = nullptr;
  // consensus Q-tables (sfl_consensus): the tables [cons_n][q_per_env] and key sets [cons_n][touched_words] of the
  // last call (cons_n == 0: none yet), and each cell's row id, built at the first call
  double* cons_q = nullptr;
  uint32_t* cons_keys = nullptr;
  uint32_t cons_n = 0;
  uint32_t* d_cell_row = nullptr;
  // step-mode learning curve (sfl_curve_*; sfl_curve.h): the ring the kernels write at episode ends, the marks, the
  // series ids and the cells, all in cv.a; the device time of the last fold and of all folds since sfl_curve_begin
  struct Curve {
    bool on = false;
    CurveArgs a{};
    float last_ms = 0.f;
    double total_ms = 0.0;
    // the exploit record (sfl_curve_exploit): x_on from the first call with f >= 1 to the curve's end;
    // x_freq is what sfl_step launches with (0 after sfl_curve_exploit(h, 0)), xa.f what the rounds are counted with;
    // x_limit [E]: the buffer xa.limit points at while x_freq == 0; the exploit fold's share of last_ms / total_ms
    bool x_on = false;
    int32_t x_freq = 0;
    CurveXArgs xa{};
    int32_t* x_limit = nullptr;
    float x_last_ms = 0.f;
    double x_total_ms = 0.0;
  } cv;
  // policy-bank evaluation (sfl_create_eval / sfl_bank_*; sfl_eval.h): on an evaluation handle st.lrn.q and
  // st.lrn.touched are null and map.bank_q / map.bank_policy point at q / policy below.  set[p]: table p was filled;
  // the per-env outputs of the last episode launch ([E], delays and at_dest [T][E]) and the cells the fold made of them
  struct Bank {
    bool on = false;
    uint32_t P = 0;
    double* q = nullptr;         // [P][q_per_env]
    uint32_t* keys = nullptr;    // [P][touched_words]
    std::vector<uint8_t> set;
    uint32_t* policy = nullptr;  // [E]
    double* cum = nullptr;
    int32_t *arrived = nullptr, *mf = nullptr, *dec = nullptr, *ticks = nullptr, *trunc = nullptr, *delays = nullptr;
    uint8_t* at_dest = nullptr;
    int64_t* cells = nullptr;    // [P][EV_WORDS]
    bool folded = false;
    float last_ms = 0.f;
    double total_ms = 0.0;
    // the non-arrival diagnosis (sfl_bank_diag*; sfl_diag.h): the tick of each train's last move, which
    // the episode launch writes beside at_dest; what the classify pass makes of it; the cells; diagnosed: the last
    // evaluation has been classified (sfl_bank_eval clears it)
    int32_t* last_move = nullptr;   // [T][E]
    uint8_t* dg_cls = nullptr;      // [T][E]
    int16_t* dg_blocker = nullptr;  // [T][E]
    int32_t* dg_sf = nullptr;       // [T][E]
    int32_t* dg_aux = nullptr;      // [2][E]
    uint32_t* dg_hot = nullptr;     // [P][H*W]
    int64_t* dg_cells = nullptr;    // [P][DG_WORDS]
    bool diagnosed = false;
    float dg_last_ms = 0.f;
    double dg_total_ms = 0.0;
    // the armed recording (sfl_bank_record*; sfl_rec.h): the listed envs on the host and the device, the
    // per-env slot index the kernels read, the frames and the decision rows, the traffic fold's output (allocated with
    // the handle); recorded: a successful sfl_bank_eval has followed the arming
    uint32_t rec_n = 0;
    int32_t rec_tick_cap = 0, rec_dec_cap = 0;
    std::vector<uint32_t> rec_env;
    uint32_t* rec_env_d = nullptr;   // [n]
    int32_t* rec_slot = nullptr;     // [E]
    int32_t* rec_cell = nullptr;     // [n][tick_cap][T]
    uint32_t* rec_bits = nullptr;    // [n][tick_cap][T]
    int32_t* rec_rows = nullptr;     // [n][dec_cap][SFL_REC_DEC_WORDS]
    uint32_t* rec_out = nullptr;     // [3 * H*W + 2 * S]
    bool recorded = false;
    float rc_last_ms = 0.f;
    double rc_total_ms = 0.0;
  } bank;
  // suspend and resume (sfl_state_*; sfl_snap.h): the fingerprint of the map descriptor (create), each
  // row's first cell and width on the host and the device (built at the first call), the pending capture between
  // sfl_state_capture and sfl_state_read (its device buffers in bufs), and the device time of the last calls
  struct Snap {
    uint64_t map_fp = 0;
    std::vector<uint8_t> row_w;
    std::vector<uint64_t> row_cell;
    uint8_t* d_row_w = nullptr;
    uint64_t* d_row_cell = nullptr;
    bool pending = false;
    SnapArgs a{};
    uint64_t n_rows = 0, n_cells = 0;
    std::vector<void*> bufs;
    float capture_ms = 0.f, restore_ms = 0.f;
  } snap;
  // external-action mode's transition assembler (sfl_env_trans_*; sfl_trans.h): on between
  // sfl_env_trans_begin and sfl_env_trans_end (or the next sfl_env_begin); a holds the ring and the assembler's own
  // state (allocated at the first begin), the step's buffers are filled in per call; parity: the cursor this call reads
  struct Trans {
    bool on = false;
    TransArgs a{};
    uint32_t parity = 0;
  } tr;

  template <class T>
  T* dalloc(size_t n) {
    if (n == 0) n = 1;
    void* p = be.alloc(n * sizeof(T));
    if (!p) return nullptr;
    allocs.push_back(p);
    return (T*)p;
  }
  template <class T>
  const T* upload(const T* src, size_t n) {
    T* d = dalloc<T>(n);
    if (d && src && n) be.h2d(d, src, n * sizeof(T));
    return d;
  }
  void dfree(void* p) {
    for (auto& a : allocs)
      if (a == p) {
        be.free(p);
        a = allocs.back();
        allocs.pop_back();
        return;
      }
  }
  ~Handle() {
    for (void* p : snap.bufs) be.free(p);
    for (void* p : allocs) be.free(p);
  }
};

// One-env-per-wavefront kernel shapes (sfl_wave.h): PPL semaphore and SPL counter registers
// per lane (ports <= 64*PPL, switches <= 64*SPL).  Index 0 = the lane-per-env kernel (k_run).
// TW: trains per env the variant's LDS prefetch records are sized for (T <= TW).
// G: lanes per env (64: one env per wavefront; 32 / 16 / 8: two / four / eight envs per wavefront, run_groups).
// OCC: waves per SIMD a grouped shape's registers are budgeted for (sfl.hip k_wave_g; 0: the G = 64 kernels' own).
#ifndef SFL_G8_OCC1
// G = 8, one train slot per lane (maps with <= 8 trains, c2: 32 envs per 256-thread block).  Round 4: c2 at 65,536
// envs 1,326 M agent-env-steps/s vs 853 M at G = 16 (profiles/r04c_c2_65536_g8.json, r04b_c2_65536_g16.json); a
// G = 8 shape with four train slots per lane for c3 spilled 100 registers at 256 VGPRs: 745 M vs 1,471 M at G = 16
// (profiles/r04c_c3_65536_g8.json), not kept
#define SFL_G8_OCC1 4
#endif
struct WaveShape {
  int PPL, SPL, TW, G, OCC;
  int LM = 0;  // 1: the map's move table and distance map are copied into the block's LDS (run_groups, round 6)
};
#ifndef SFL_LM_OCC
#define SFL_LM_OCC 4  // variant 11's register budget (waves per SIMD)
#endif
#ifndef SFL_V7_OCC
#define SFL_V7_OCC 4  // variant 7 (c3): waves per SIMD its registers are budgeted for (tuning builds: 3)
#endif
constexpr WaveShape kVariants[] = {{0, 0, 0, 64, 0},    {1, 1, 32, 64, 0},  {4, 1, 32, 64, 0}, {4, 1, 64, 64, 0},
                                   {8, 2, 64, 64, 0},   {16, 4, 128, 64, 0}, {4, 1, 16, 16, 4}, {16, 4, 32, 16, SFL_V7_OCC},
                                   {2, 1, 32, 32, 4},   {8, 2, 32, 32, 4},   {8, 2, 8, 8, SFL_G8_OCC1},
                                   {2, 1, 32, 32, SFL_LM_OCC, 1}};
constexpr int kNumVariants = 12;
// Variant 11 = variant 8 with the map's move table and distance map (as int16) in LDS (LM): a batch of at most two
// wavefronts per SIMD (kLmWaves; configs[1], c2 at 4,096 envs: 2,048 wavefronts at G = 32) runs two 256-thread blocks
// per CU, which leaves each block ~63 KB of LDS beyond its env records; the tick's two move-table lookups and the
// staging's move-table and distance lookups then become LDS reads instead of dependent L2 round trips.  Chosen where
// the tables fit kLmBytes (c2: 40,000 + 20,000 bytes); SFL_LDS_MAP=0 keeps variant 8.
constexpr uint64_t kLmWaves = 2048;
constexpr int64_t kLmBytes = 64512;  // (sfl_wave.h run_groups: LM_WORDS)
inline int64_t lm_bytes(const sfl_map_desc* md) {
  const int64_t hw = (int64_t)md->H * md->W;
  return hw * 4 * 16 + ((int64_t)md->K * hw * 4 + 1) / 2 * 4;
}
#ifndef SFL_DEFAULT_G
#define SFL_DEFAULT_G 16  // lane group size chosen where a grouped shape fits (SFL_WAVE_G overrides)
#endif

// Eligibility: trains fit one or two slots per lane (T <= 128), the env fits the variant's
// registers and every semaphore record fits the 32-bit LDS word (sfl_wave.h r_pack: start tick
// -8192..8191, span <= 511).  SFL_KERNEL=scalar forces k_run.  why: when non-null, the reason a
// map is not eligible (the caller reports it; the lane-per-env body is 15-45x slower).
// A batch too small to fill the device at the default group size (fewer than kFillWaves wavefronts: 4 per SIMD
// of MI355X's 1,024) takes two envs per wavefront instead of four: c2 at its stated 4,096 envs 316 M vs 276 M
// agent-env-steps/s (G = 64: 313 M), while c3 at 16,384 envs -- 4,096 wavefronts at G = 16 -- keeps G = 16
// (1,275 M vs 982 M at G = 64; profiles/r03d_group_size_*.json).  Round 4, c2 at 4,096 envs: G = 8 229 M, 16 291 M,
// 32 326 M, 64 323 M (profiles/r04c_c2_4096_g*.json).
constexpr uint64_t kFillWaves = 4096;
inline int choose_variant(const sfl_map_desc* md, bool backend_has_wave, std::string* why = nullptr, uint64_t n_envs = 0) {
  if (!backend_has_wave) return 0;
  const char* env = getenv("SFL_KERNEL");
  if (env && strcmp(env, "scalar") == 0) return 0;
  auto no = [&](const char* r) {
    if (why) *why = r;
    return 0;
  };
  if (md->T > 128) return no("more than 128 trains");
  int32_t ed_max = 0, ed_min = 0, dist_max = 0, len_max = 0;
  for (int32_t h = 0; h < md->T; ++h) {
    ed_max = md->tr_ed[h] > ed_max ? md->tr_ed[h] : ed_max;
    ed_min = md->tr_ed[h] < ed_min ? md->tr_ed[h] : ed_min;
    dist_max = md->tr_init_dist[h] > dist_max ? md->tr_init_dist[h] : dist_max;
  }
  for (int32_t p = 0; p < md->S * 4; ++p) len_max = md->port_len[p] > len_max ? md->port_len[p] : len_max;
  const int64_t span = (int64_t)(dist_max > 2 * len_max + 2 ? dist_max : 2 * len_max + 2) + 4;
  const int64_t t_hi = (int64_t)(ed_max > md->max_episode_steps ? ed_max : md->max_episode_steps) + 2 + span;
  if (t_hi > 8191 || ed_min - 2 < -8192) return no("timetable horizon beyond 8191 ticks");
  if (span > 511) return no("a semaphore span beyond 511 ticks");
  for (size_t i = 0, n = (size_t)md->K * md->H * md->W * 4; i < n; ++i)  // (staged as int16, sfl_wave.h d16)
    if (md->dist[i] >= 32767 && md->dist[i] < DIST_INF) return no("a finite distance of 32767 cells or more");
  if (md->q_per_env >= (1ull << 32)) return no("Q-table beyond 2^32 cells per env");
  if ((int64_t)md->H * md->W >= (1 << 20) - 1) return no("grid beyond 2^20 cells");
  const char* gs = getenv("SFL_WAVE_G");
  // one train per lane, eight envs per wavefront, for maps with <= 8 trains (round 4)
  int want_g = gs ? atoi(gs) : (md->T <= 8 ? 8 : SFL_DEFAULT_G);
  if (!gs && n_envs > 0 && want_g < 32 && n_envs * (uint64_t)want_g / 64 < kFillWaves) want_g = 32;
  auto fits = [&](int v) {
    const WaveShape& w = kVariants[v];
    return md->S * 4 <= w.G * w.PPL && md->S <= w.G * w.SPL && md->T <= w.TW;
  };
  const char* lms = getenv("SFL_LDS_MAP");
  const bool lm_ok = !(lms && atoi(lms) == 0) && n_envs > 0 && n_envs * (uint64_t)want_g / 64 <= kLmWaves &&
                     lm_bytes(md) <= kLmBytes;
  for (int v = 1; v < kNumVariants; ++v) {
    if (kVariants[v].LM || kVariants[v].G != want_g || !fits(v)) continue;
    if (lm_ok)  // the same shape with the map tables in LDS, if there is one
      for (int u = 1; u < kNumVariants; ++u) {
        const WaveShape &a = kVariants[u], &b = kVariants[v];
        if (a.LM && a.PPL == b.PPL && a.SPL == b.SPL && a.TW == b.TW && a.G == b.G) return u;
      }
    return v;
  }
  for (int v = 1; v < kNumVariants; ++v)
    if (kVariants[v].G == 64 && fits(v)) return v;
  return no("more than 256 switches");
}

// the one-env-per-wavefront shape of the same map (the partitioned local step runs G = 64 only)
inline int wave64_variant(int S, int T) {
  for (int v = 1; v < kNumVariants; ++v) {
    const WaveShape& w = kVariants[v];
    if (w.G == 64 && S * 4 <= w.G * w.PPL && S <= w.G * w.SPL && T <= w.TW) return v;
  }
  return 0;
}

// n_policies > 0: an evaluation handle (sfl_create_eval) -- no per-env Q block and key set, a bank of n_policies tables
template <class B>
int create(const sfl_map_desc* md, const sfl_hparams* hp, uint32_t n_envs, const uint64_t* env_seeds, int device,
           Handle<B>** out, uint32_t n_policies = 0) {
  const std::string fn = n_policies ? "sfl_create_eval" : "sfl_create";  // (the entry point the messages name)
  if (!md || !hp || !out || n_envs == 0) return fail(fn + ": null argument or zero envs");
  if (md->T > 32 * MAXW) return fail(fn + ": at most 128 trains per env");
  if (md->S * 4 >= 0xFFFF) return fail(fn + ": too many switches");
  if (md->K < 1 || md->K > 341) return fail(fn + ": station count out of range");
  if (md->delay_threshold < -65536 || md->delay_threshold > 65536) return fail(fn + ": delay_threshold out of range");
  auto* h = new Handle<B>();
  h->device = device;
  if (int rc = h->be.init(device)) {
    const std::string why = h->be.error();
    delete h;
    return fail(fn + ": backend init failed: " + why);
  }
  h->E = n_envs;
  h->h_sw_np.assign(md->sw_np, md->sw_np + md->S);
  h->h_q_w.assign(md->q_w, md->q_w + (size_t)md->S * 4);
  h->h_q_off.assign(md->q_off, md->q_off + (size_t)md->S * 4);
  h->h_row_base.assign(md->row_base, md->row_base + (size_t)md->S * 4);
  h->variant = h->created_variant = choose_variant(md, B::kHasWave, &h->variant_note, n_envs);
  SflMap& m = h->map;
  const size_t HW = (size_t)md->H * md->W, NP = (size_t)md->S * 4, S = md->S, T = md->T;
  m.H = md->H;
  m.W = md->W;
  m.HW = md->H * md->W;
  m.cell_bits = 1;
  while ((1 << m.cell_bits) < m.HW) ++m.cell_bits;
  m.lrn.S = md->S;
  m.T = md->T;
  m.lrn.ST = md->S * md->T;
  m.dec.K = md->K;
  m.NP = (int32_t)NP;
  m.max_episode_steps = md->max_episode_steps;
  m.mf_rate = md->mf_rate;
  m.mf_min = md->mf_min;
  m.mf_max = md->mf_max;
  mf_prepare(m);  // (mf_propose's integer forms of u < mf_rate and of the duration's modulo)
  m.dec.delay_thr = md->delay_threshold;
  m.upd.gamma = hp->gamma;
  m.eps0 = hp->epsilon;
  m.eps_decay = hp->epsilon_decay_rate;
  // (log2 of 0 is -inf and of a negative value NaN: the device test is then never certain and takes the table)
  m.upd.lr0 = hp->lr;
  m.upd.lr_decay = hp->lr_decay_rate;
  m.dec.default_q = hp->default_q;
  m.max_steps = hp->max_steps;
  m.lrn.ntab = hp->ntab;
  m.lrn.q_per_env = md->q_per_env;
  m.rows_per_env = md->rows_per_env;
  m.lrn.touched_words = (md->rows_per_env + 31u) / 32u;
  m.grid = h->upload(md->grid, HW);
  m.cell_sw = h->upload(md->cell_sw, HW);
  m.sw_np = h->upload(md->sw_np, S);
  m.sw_na = h->upload(md->sw_na, S);
  m.act_src = h->upload(md->act_src, S * 8);
  m.act_dst = h->upload(md->act_dst, S * 8);
  m.act_turn = h->upload(md->act_turn, S * 8);
  m.act_j = h->upload(md->act_j, S * 8);
  m.first_other = h->upload(md->first_other, NP);
  m.port_side = h->upload(md->port_side, NP);
  m.slot_nroutes = h->upload(md->slot_nroutes, NP);
  m.slot_route_act = h->upload(md->slot_route_act, NP * 4);
  m.q_w = h->upload(md->q_w, NP);
  m.port_nb = h->upload(md->port_nb, NP);
  m.port_len = h->upload(md->port_len, NP);
  m.port_unique = h->upload(md->port_unique, NP);
  m.q_off = h->upload(md->q_off, NP);
  m.row_base = h->upload(md->row_base, NP);
  m.dist = h->upload(md->dist, (size_t)md->K * HW * 4);
  m.tr_ed = h->upload(md->tr_ed, T);
  m.tr_la = h->upload(md->tr_la, T);
  m.tr_k = h->upload(md->tr_k, T);
  m.tr_target = h->upload(md->tr_target, T);
  m.tr_init_cell = h->upload(md->tr_init_cell, T);
  m.tr_init_dist = h->upload(md->tr_init_dist, T);
  m.tr_init_delay = h->upload(md->tr_init_delay, T);
  m.tr_init_dir = h->upload(md->tr_init_dir, T);
  m.tr_init_port = h->upload(md->tr_init_port, T);
  m.dec.eps_tab = h->upload(hp->eps_tab, (size_t)hp->ntab);
  m.lrn.lr_tab = h->upload(hp->lr_tab, (size_t)hp->ntab);
  {
    // the observation vector's coordinates (observer.py:303-306: the switch cell, the target station's cell): the
    // switch of a cell is cell_sw, every station is some train's target (compiler.py builds the stations from them)
    std::vector<uint32_t> sw_rc(S * 2, 0xFFFFFFFFu), st_rc((size_t)md->K * 2, 0xFFFFFFFFu);
    for (size_t cell = 0; cell < HW; ++cell) {
      const int sw = md->cell_sw[cell];
      if (sw >= 0 && (size_t)sw < S) {
        sw_rc[2 * sw] = (uint32_t)(cell / (size_t)md->W);
        sw_rc[2 * sw + 1] = (uint32_t)(cell % (size_t)md->W);
      }
    }
    for (size_t t = 0; t < T; ++t) {
      const int k = md->tr_k[t], cell = md->tr_target[t];
      if (k >= 0 && k < md->K && cell >= 0) {
        st_rc[2 * k] = (uint32_t)(cell / md->W);
        st_rc[2 * k + 1] = (uint32_t)(cell % md->W);
      }
    }
    for (size_t sw = 0; sw < S; ++sw) h->max_na = std::max(h->max_na, (int)md->sw_na[sw]);
    h->keep.push_back(std::move(sw_rc));
    h->d_sw_rc = (int32_t*)h->upload(h->keep.back().data(), S * 2);
    h->keep.push_back(std::move(st_rc));
    h->d_st_rc = (int32_t*)h->upload(h->keep.back().data(), (size_t)md->K * 2);
  }
  {
    // packed tables for the one-env-per-wave kernel: one scalar load per switch / port / train,
    // and check_action as a table lookup
    std::vector<uint32_t> swp(S * 16, 0), pp(NP * 4, 0), mv(HW * 16, 0);
    std::vector<int32_t> trp(T * 8, 0);
    bool pack_ok = true;
    for (size_t sw = 0; sw < S; ++sw) {
      uint32_t* w = &swp[sw * 16];
      const int na = md->sw_na[sw];
      w[0] = (uint32_t)md->sw_np[sw] | ((uint32_t)na << 4);
      for (int a = 0; a < 8 && a < na - 1; ++a) {  // routes (STOP = action na-1 has no entry)
        w[1] |= ((uint32_t)md->act_src[sw * 8 + a] & 3u) << (2 * a);
        w[1] |= ((uint32_t)md->act_dst[sw * 8 + a] & 3u) << (16 + 2 * a);
        w[2] |= ((uint32_t)md->act_turn[sw * 8 + a] & 3u) << (2 * a);
        w[2] |= ((uint32_t)md->act_j[sw * 8 + a] & 3u) << (16 + 2 * a);
      }
      for (int sl = 0; sl < 4; ++sl) {
        const uint32_t qw = md->q_w[sw * 4 + sl];
        w[3] |= (qw & 15u) << (4 * sl);
        // compact row descriptor: full-row action of each compact column (routes leaving
        // through this slot in action order, then STOP), and the first default-valued action
        uint32_t rd = 0, c = 0, mind = 15;
        for (int a = 0; a < na - 1; ++a) {
          if (md->act_src[sw * 8 + a] == sl) {
            if (md->act_j[sw * 8 + a] != c) rd |= 1u << 31;  // columns must follow action order
            rd |= ((uint32_t)a & 15u) << (4 * c++);
          } else if (mind == 15) {
            mind = (uint32_t)a;
          }
        }
        if (qw > 0) {
          if (c != qw - 1u) rd |= 1u << 31;
          rd |= ((uint32_t)(na - 1) & 15u) << (4 * c);
        }
        rd |= mind << 16;
        if (rd >> 31) pack_ok = false;
        w[4 + sl] = rd;
        // neighbour port of each port (observer lanes)
        w[8 + (sl >> 1)] |= (uint32_t)(uint16_t)md->port_nb[sw * 4 + sl] << (16 * (sl & 1));
      }
    }
    for (size_t p = 0; p < NP; ++p) {
      pp[p * 4 + 0] = (uint32_t)(uint16_t)md->port_nb[p] | ((uint32_t)(uint16_t)md->port_len[p] << 16);
      pp[p * 4 + 1] = (uint32_t)(uint16_t)md->port_unique[p] | ((uint32_t)md->q_w[p] << 16);
      pp[p * 4 + 2] = md->row_base[p];
      pp[p * 4 + 3] = (uint32_t)md->q_off[p];
    }
    std::vector<uint32_t> ptr_(NP * 4, 0);
    for (size_t o = 0; o < NP; ++o) {
      const int t = md->port_nb[o];
      const int u = t >= 0 ? md->port_unique[t] : -1;
      const int far = u >= 0 ? md->port_nb[u] : -1;
      ptr_[o * 4 + 0] = (uint32_t)(uint16_t)(int16_t)t | ((uint32_t)(uint16_t)(int16_t)u << 16);
      ptr_[o * 4 + 1] = (uint32_t)(uint16_t)(int16_t)far | ((uint32_t)(uint16_t)md->port_len[o] << 16);
      ptr_[o * 4 + 2] = u >= 0 ? (uint32_t)(uint16_t)md->port_len[u] : 0u;
    }
    for (size_t c = 0; c < HW; ++c)
      for (int d = 0; d < 4; ++d)
        for (int a = 0; a < 4; ++a)
        {
          // bits 24-31: the switch at the destination cell (0xFF: none, or more than 254 switches)
          uint32_t w = move_pack(md->grid, md->H, md->W, (uint32_t)a, (int)c, d);
          const int nc = (int)(w & 0xFFFFFu) - 1;
          const int swd = nc >= 0 ? md->cell_sw[nc] : -1;
          w |= (uint32_t)(swd >= 0 && md->S <= 254 ? swd : 0xFF) << 24;
          mv[(c * 4 + d) * 4 + a] = w;
        }
    for (size_t t = 0; t < T; ++t) {
      int32_t* w = &trp[t * 8];
      w[0] = md->tr_ed[t];
      w[1] = md->tr_la[t];
      w[2] = md->tr_k[t];
      w[3] = md->tr_target[t];
      w[4] = md->tr_init_cell[t];
      w[5] = md->tr_init_dist[t];
      w[6] = md->tr_init_delay[t];
      w[7] = (int32_t)((uint32_t)md->tr_init_dir[t] | ((uint32_t)(uint16_t)md->tr_init_port[t] << 16));
    }
    if (!pack_ok) {
      delete h;
      return fail(fn + ": compact Q columns do not follow action order (map compiler mismatch)");
    }
    h->keep.push_back(std::move(swp));
    m.sw_pack = h->upload(h->keep.back().data(), h->keep.back().size());
    h->keep.push_back(std::move(pp));
    m.port_pack = h->upload(h->keep.back().data(), h->keep.back().size());
    // two steps ahead (the batch prefetch's reward projections, sfl_wave.h prefetch_slot)
    std::vector<uint32_t> mv2c(HW * 64, 0u);
    for (size_t i = 0; i < HW * 16; ++i) {
      const int nc = (int)(mv[i] & 0xFFFFFu) - 1, nd = (int)((mv[i] >> 20) & 3u);
      for (int n = 0; n < 4; ++n) mv2c[i * 4 + n] = nc < 0 ? ((uint32_t)nd << 20) : mv[((size_t)nc * 4 + nd) * 4 + n];
    }
    h->keep.push_back(std::move(mv));
    m.move_tab = h->upload(h->keep.back().data(), h->keep.back().size());
    h->keep.push_back(std::move(mv2c));
    m.move2c_tab = h->upload(h->keep.back().data(), h->keep.back().size());
    h->keep.push_back(std::move(ptr_));
    m.port_tr = h->upload(h->keep.back().data(), h->keep.back().size());
    m.dec.seedseq32 = h->be.seedseq_table();
    h->keep.emplace_back(trp.begin(), trp.end());
    m.tr_pack = (const int32_t*)h->upload(h->keep.back().data(), h->keep.back().size());
  }

  SflState& s = h->st;
  const size_t E = n_envs;
  s.E = n_envs;
  s.phase = h->template dalloc<int32_t>(E);
  s.elapsed = h->template dalloc<int32_t>(E);
  s.eflags = h->template dalloc<uint32_t>(E);
  s.ep_t = h->template dalloc<int32_t>(E);
  s.n_test = h->template dalloc<int32_t>(E);
  s.epoch = h->template dalloc<uint32_t>(E);
  s.rng = h->template dalloc<uint64_t>(5 * E);
  s.seed = h->template dalloc<uint64_t>(E);
  s.cum_reward = h->template dalloc<double>(E);
  s.n_mf = h->template dalloc<int32_t>(E);
  s.ep_dec = h->template dalloc<int32_t>(E);
  s.ep_ticks = h->template dalloc<int32_t>(E);
  s.step_ctr = h->template dalloc<int64_t>(E);
  s.dec_total = h->template dalloc<int64_t>(E);
  s.masks = h->template dalloc<uint32_t>(4 * MAXW * E);
  s.err = h->template dalloc<uint32_t>(E);
  s.tr_pos = h->template dalloc<int32_t>(T * E);
  s.tr_bits = h->template dalloc<uint32_t>(T * E);
  s.tr_plan = h->template dalloc<uint32_t>(T * E);
  s.tr_next = h->template dalloc<uint16_t>(T * E);
  s.tr_prev = h->template dalloc<uint16_t>(T * E);
  s.tr_src = h->template dalloc<uint16_t>(T * E);
  s.tr_dec = h->template dalloc<uint16_t>(T * E);
  s.tr_delay = h->template dalloc<int32_t>(T * E);
  s.own = h->template dalloc<uint16_t>(T * OWN_MAX * E);
  s.own_n = h->template dalloc<uint8_t>(T * E);
  s.sc_desired = h->template dalloc<int32_t>(T * E);
  s.sc_pred = h->template dalloc<int32_t>(T * E);
  s.sc_aux = h->template dalloc<uint32_t>(T * E);
  s.occ = h->template dalloc<uint8_t>(HW * E);
  s.claim = h->template dalloc<uint8_t>(HW * E);
  s.sem = h->template dalloc<uint64_t>(NP * E);
  s.lrn.slot = h->template dalloc<uint64_t>(S * T * E);
  s.lrn.counts = h->template dalloc<uint32_t>(S * E);
  typename Handle<B>::Bank& bk = h->bank;
  bk.on = n_policies > 0;
  if (!bk.on) {
    s.lrn.q = h->template dalloc<double>((size_t)m.lrn.q_per_env * E);
    s.lrn.touched = h->template dalloc<uint32_t>((size_t)m.lrn.touched_words * E);
  } else {
    bk.P = n_policies;
    bk.set.assign(n_policies, 0);
    bk.q = h->template dalloc<double>((size_t)m.lrn.q_per_env * n_policies);
    bk.keys = h->template dalloc<uint32_t>((size_t)m.lrn.touched_words * n_policies);
    bk.policy = h->template dalloc<uint32_t>(E);
    bk.cum = h->template dalloc<double>(E);
    bk.arrived = h->template dalloc<int32_t>(E);
    bk.mf = h->template dalloc<int32_t>(E);
    bk.dec = h->template dalloc<int32_t>(E);
    bk.ticks = h->template dalloc<int32_t>(E);
    bk.trunc = h->template dalloc<int32_t>(E);
    bk.delays = h->template dalloc<int32_t>(T * E);
    bk.at_dest = h->template dalloc<uint8_t>(T * E);
    bk.cells = h->template dalloc<int64_t>((size_t)n_policies * EV_WORDS);
    bk.last_move = h->template dalloc<int32_t>(T * E);
    bk.dg_cls = h->template dalloc<uint8_t>(T * E);
    bk.dg_blocker = h->template dalloc<int16_t>(T * E);
    bk.dg_sf = h->template dalloc<int32_t>(T * E);
    bk.dg_aux = h->template dalloc<int32_t>(2 * E);
    bk.dg_hot = h->template dalloc<uint32_t>((size_t)n_policies * HW);
    bk.dg_cells = h->template dalloc<int64_t>((size_t)n_policies * DG_WORDS);
    bk.rec_out = h->template dalloc<uint32_t>(3 * (size_t)HW + 2 * (size_t)m.lrn.S);
    m.bank_q = bk.q;
    m.bank_policy = bk.policy;
  }
  h->d_launch_dec = h->template dalloc<uint64_t>(E);
  h->d_launch_ticks = h->template dalloc<uint64_t>(E);
  h->d_launch_bytes = h->template dalloc<uint64_t>(E);
  h->d_sums = h->template dalloc<uint64_t>(4);
  h->d_phase = h->template dalloc<uint64_t>(8);
  for (void* p : h->allocs)
    if (!p) {
      delete h;
      return fail(fn + ": device allocation failed");
    }
  if (!m.grid || (!bk.on && !s.lrn.q) || (bk.on && !bk.q)) {
    delete h;
    return fail(fn + ": device allocation failed (out of memory?)");
  }
  // initial values
  h->be.memset(s.phase, 0, E * 4);
  h->be.memset(s.elapsed, 0, E * 4);
  h->be.memset(s.eflags, 0, E * 4);
  h->be.memset(s.ep_t, 0, E * 4);
  h->be.memset(s.n_test, 0, E * 4);
  h->be.memset(s.epoch, 0, E * 4);
  h->be.memset(s.rng, 0, 5 * E * 8);
  h->be.memset(s.cum_reward, 0, E * 8);
  h->be.memset(s.n_mf, 0, E * 4);
  h->be.memset(s.ep_dec, 0, E * 4);
  h->be.memset(s.ep_ticks, 0, E * 4);
  h->be.memset(s.step_ctr, 0, E * 8);
  h->be.memset(s.dec_total, 0, E * 8);
  h->be.memset(s.masks, 0, 4 * MAXW * E * 4);
  h->be.memset(s.err, 0, E * 4);
  h->be.memset(s.tr_pos, 0xFF, T * E * 4);  // -1: off map
  h->be.memset(s.tr_bits, 0, T * E * 4);
  h->be.memset(s.tr_plan, 0, T * E * 4);
  h->be.memset(s.tr_next, 0, T * E * 2);
  h->be.memset(s.tr_prev, 0xFF, T * E * 2);  // None
  h->be.memset(s.tr_src, 0xFF, T * E * 2);   // None
  h->be.memset(s.tr_dec, 0, T * E * 2);
  h->be.memset(s.tr_delay, 0, T * E * 4);
  h->be.memset(s.own_n, 0, T * E);
  // (never read before they are written; zeroed so that a state record, sfl_state_capture, is a function of the run
  // and not of what the allocator handed out: the wave kernels never write these four)
  h->be.memset(s.own, 0, T * OWN_MAX * E * 2);
  h->be.memset(s.sc_desired, 0, T * E * 4);
  h->be.memset(s.sc_pred, 0, T * E * 4);
  h->be.memset(s.sc_aux, 0, T * E * 4);
  h->be.memset(s.occ, 0xFF, HW * E);
  h->be.memset(s.claim, 0xFF, HW * E);
  h->be.memset(s.sem, 0, NP * E * 8);
  h->be.memset(s.lrn.slot, 0, S * T * E * 8);
  h->be.memset(s.lrn.counts, 0, S * E * 4);
  h->be.memset(h->d_phase, 0, 8 * 8);
  if (!bk.on) {
    h->be.memset(s.lrn.touched, 0, (size_t)m.lrn.touched_words * E * 4);
    h->be.fill_f64(s.lrn.q, m.dec.default_q, (size_t)m.lrn.q_per_env * E);
  } else {
    h->be.memset(bk.keys, 0, (size_t)m.lrn.touched_words * bk.P * 4);
    h->be.fill_f64(bk.q, m.dec.default_q, (size_t)m.lrn.q_per_env * bk.P);
    h->be.memset(bk.policy, 0, E * 4);
  }
  h->seeds.assign(env_seeds, env_seeds + E);
  h->snap.map_fp = snap_map_fp(md);
  h->be.h2d(s.seed, env_seeds, E * 8);
  if (int rc = h->be.sync()) {
    delete h;
    return fail((fn + ": ") + h->be.error());
  }
  *out = h;
  return 0;
}

// Flatland-compatible malfunction stream: table[E][steps][T] proposals (sfl_mfgen.h); steps == 0
// returns to the counter-based draw
template <class B>
int set_mf_schedule(Handle<B>* h, int32_t steps, const uint8_t* table) {
  SflMap& m = h->map;
  if (steps < 0 || (steps > 0 && !table)) return fail("sfl_set_mf_schedule: bad argument");
  if (steps > 0 && m.seed_sched)
    return fail("sfl_set_mf_schedule: the handle has a seed schedule (sfl_set_seed_schedule), which keys the counter-based draw");
  if (m.mf_tab) {
    h->dfree((void*)m.mf_tab);
    m.mf_tab = nullptr;
  }
  m.mf_steps = 0;
  if (steps == 0) return 0;
  const size_t n = (size_t)h->E * (size_t)steps * (size_t)m.T;
  // (a byte is the train's malfunction counter field, tb_mf)
  m.mf_tab = h->upload(table, n);
  if (!m.mf_tab) return fail("sfl_set_mf_schedule: device allocation failed");
  m.mf_steps = steps;
  return h->be.sync() ? fail(h->be.error()) : 0;
}

// Hyperparameter groups (include/sfl.h sfl_set_hparam_groups): the groups' tables as [n_groups][ntab], their
// scalars as [n_groups][4] (HPG_*) and env_group[E] in device memory; the kernels read them from the next launch.
// Everything is validated on the host before anything is uploaded; a refused call leaves the handle as it was.
template <class B>
int set_hparam_groups(Handle<B>* h, int32_t n_groups, const sfl_hparam_group* groups, const uint16_t* env_group) {
  if (h->bank.on) return fail("sfl_set_hparam_groups: an evaluation handle has no learner (sfl_create_eval)");
  if (h->part.world) return fail("sfl_set_hparam_groups: the handle is graph-partitioned");
  if (h->env_mode) return fail("sfl_set_hparam_groups: the handle is in external-action mode (no learner)");
  if (n_groups < 0 || n_groups > SFL_MAX_HPARAM_GROUPS)
    return fail("sfl_set_hparam_groups: n_groups outside [0, " + std::to_string(SFL_MAX_HPARAM_GROUPS) + "]");
  SflMap& m = h->map;
  const size_t ntab = m.lrn.ntab > 0 ? (size_t)m.lrn.ntab : 0, G = (size_t)n_groups, E = h->E;
  const double *d_eps = nullptr, *d_lr = nullptr, *d_sc = nullptr;
  const uint16_t* d_eg = nullptr;
  if (n_groups > 0) {
    if (!groups || !env_group) return fail("sfl_set_hparam_groups: null groups or env_group");
    for (size_t g = 0; g < G; ++g)
      if (ntab && (!groups[g].eps_tab || !groups[g].lr_tab))
        return fail("sfl_set_hparam_groups: group " + std::to_string(g) + " has a null table");
    for (size_t e = 0; e < E; ++e)
      if (env_group[e] >= n_groups)
        return fail("sfl_set_hparam_groups: env " + std::to_string(e) + " is in group " + std::to_string(env_group[e]) +
                    " of " + std::to_string(n_groups));
    std::vector<double> eps(G * ntab), lr(G * ntab), sc(G * 4);
    for (size_t g = 0; g < G; ++g) {
      if (ntab) {
        memcpy(&eps[g * ntab], groups[g].eps_tab, ntab * 8);
        memcpy(&lr[g * ntab], groups[g].lr_tab, ntab * 8);
      }
      sc[g * 4 + HPG_EPS0] = groups[g].epsilon;
      sc[g * 4 + HPG_EPS_DECAY] = groups[g].epsilon_decay_rate;
      sc[g * 4 + HPG_LR0] = groups[g].lr;
      sc[g * 4 + HPG_LR_DECAY] = groups[g].lr_decay_rate;
    }
    d_eps = h->upload(eps.data(), eps.size());
    d_lr = h->upload(lr.data(), lr.size());
    d_sc = h->upload(sc.data(), sc.size());
    d_eg = h->upload(env_group, E);
    const bool ok = d_eps && d_lr && d_sc && d_eg && h->be.sync() == 0;  // (the host sources live until here)
    if (!ok) {
      for (const void* p : {(const void*)d_eps, (const void*)d_lr, (const void*)d_sc, (const void*)d_eg})
        if (p) h->dfree((void*)p);
      return fail(std::string("sfl_set_hparam_groups: device allocation or upload failed") +
                  (h->be.error()[0] ? std::string(": ") + h->be.error() : std::string()));
    }
  } else if (h->be.sync()) {
    return fail(h->be.error());
  }
  // (synchronous API: no launch of the handle is in flight, the old arrays can go)
  for (const void* p : {(const void*)m.hpg_eps_tab, (const void*)m.hpg_lr_tab, (const void*)m.hpg_sc, (const void*)m.env_group})
    if (p) h->dfree((void*)p);
  m.n_groups = n_groups;
  m.hpg_eps_tab = d_eps;
  m.hpg_lr_tab = d_lr;
  m.hpg_sc = d_sc;
  m.env_group = d_eg;
  return 0;
}

// Seed schedules (include/sfl.h sfl_set_seed_schedule).  The schedule lives in the map (seed_sched,
// seed_pool, seed_flags); the seed of the episode each env started last in SflState::ep_seed, allocated by the first
// call that leaves the default and filled with the base seeds -- the episodes in flight run on them to their end.
// From then on the handle launches the scheduled kernels, also after a return to pool 1 / flags 0 (which they run as
// the rule states it: every episode on the base seed), so that a call always takes effect at each env's next reset.
// Everything is validated before anything changes.
template <class B>
int set_seed_schedule(Handle<B>* h, uint32_t pool, uint32_t flags) {
  const std::string fn = "sfl_set_seed_schedule: ";
  if (h->bank.on)
    return fail(fn + "an evaluation handle's seeds are chosen at create (sfl_create_eval); derive them with sfl_episode_seed");
  if (h->part.world) return fail(fn + "the handle is graph-partitioned");
  if (h->map.mf_steps > 0)
    return fail(fn + "the handle has a Flatland malfunction table (sfl_set_mf_schedule), which no seed keys");
  if (pool > 0x7FFFFFFFu) return fail(fn + "pool " + std::to_string(pool) + " beyond 2^31 - 1");
  if (flags & ~SEED_HELDOUT_EXPLOIT) return fail(fn + "unknown flag bits " + std::to_string(flags & ~SEED_HELDOUT_EXPLOIT));
  if (h->env_mode && (flags & SEED_HELDOUT_EXPLOIT))
    return fail(fn + "SFL_SEED_HELDOUT_EXPLOIT in external-action mode, where no episode is greedy");
  SflMap& m = h->map;
  if (!m.seed_sched && pool == 1 && flags == 0) return 0;  // the default on a handle that never left it
  const size_t E = h->E;
  if (!m.seed_sched) {
    if (!h->st.ep_seed) h->st.ep_seed = h->template dalloc<uint64_t>(E);
    if (!h->st.ep_seed) return fail(fn + "device allocation failed");
    h->be.h2d(h->st.ep_seed, h->seeds.data(), E * 8);
    if (h->env_mode) {
      // external-action mode counts started episodes in ep_t from here: an env that stands at its reset starts
      // episode 0 there, the episode in flight of any other is episode 0
      std::vector<int32_t> ph(E), t(E);
      h->be.d2h(ph.data(), h->st.phase, E * 4);
      if (h->be.sync()) return fail(fn + h->be.error());
      for (size_t e = 0; e < E; ++e) t[e] = ph[e] == PH_RESET ? -1 : 0;
      h->be.h2d(h->st.ep_t, t.data(), E * 4);
    }
    if (h->be.sync()) return fail(fn + h->be.error());
  }
  m.seed_sched = 1;
  m.seed_pool = pool;
  m.seed_flags = flags;
  return 0;
}

template <class B>
int get_seed_schedule(Handle<B>* h, uint32_t* pool, uint32_t* flags) {
  if (pool) *pool = h->map.seed_sched ? h->map.seed_pool : 1u;
  if (flags) *flags = h->map.seed_sched ? h->map.seed_flags : 0u;
  return 0;
}

template <class B>
int get_episode_seeds(Handle<B>* h, uint64_t* out) {
  if (!out) return fail("sfl_get_episode_seeds: null argument");
  if (!h->map.seed_sched) {
    memcpy(out, h->seeds.data(), (size_t)h->E * 8);
    return 0;
  }
  h->be.d2h(out, h->st.ep_seed, (size_t)h->E * 8);
  return h->be.sync() ? fail(std::string("sfl_get_episode_seeds: ") + h->be.error()) : 0;
}

template <class B>
int part_host_access(Handle<B>* h, bool write);
template <class B>
int curve_exploit_sync(Handle<B>* h);

// rng_states: [E][5] (state hi, state lo, inc hi, inc lo, has<<32|buf) — numpy's
// default_rng(seed).bit_generator.state, computed on the host.
template <class B>
int learn_begin(Handle<B>* h, const uint64_t* rng_states) {
  if (h->bank.on) return fail("sfl_learn_begin: an evaluation handle has no learner (sfl_create_eval)");
  if (int rc = part_host_access(h, true)) return rc;
  const size_t E = h->E;
  std::vector<uint64_t> soa(5 * E);
  for (size_t e = 0; e < E; ++e)
    for (int k = 0; k < 5; ++k) soa[k * E + e] = rng_states[e * 5 + k];
  h->be.h2d(h->st.rng, soa.data(), soa.size() * 8);
  h->be.memset(h->st.lrn.counts, 0, (size_t)h->map.lrn.S * E * 4);
  h->be.memset(h->st.ep_t, 0, E * 4);
  if (h->map.seed_sched) h->be.h2d(h->st.ep_seed, h->seeds.data(), E * 8);  // (the base seed before the first reset)
  // every env starts the learn() call with a fresh reset, and no exploit round done yet
  std::vector<int32_t> ph(E, PH_RESET);
  h->be.h2d(h->st.phase, ph.data(), E * 4);
  std::vector<uint32_t> fl(E);
  h->be.d2h(fl.data(), h->st.eflags, E * 4);
  for (auto& f : fl) f &= ~(F_EXPLOIT_DONE | F_INFLIGHT | F_GREEDY);
  h->be.h2d(h->st.eflags, fl.data(), E * 4);
  if (h->cv.on) {  // the curve starts over with the episode indices: marks at 0, cells empty
    h->be.memset(h->cv.a.mark, 0, E * 4);
    if (h->be.curve(h->cv.a, true)) return fail(std::string("sfl_learn_begin: ") + h->be.error());
    if (h->cv.x_on) {  // and so does the exploit record: no round completed, none in flight
      if (h->be.curve_exploit(h->cv.xa, true)) return fail(std::string("sfl_learn_begin: ") + h->be.error());
      if (int rc = curve_exploit_sync(h)) return rc;
    }
  }
  return h->be.sync() ? fail(h->be.error()) : 0;
}

template <class B>
int test_begin(Handle<B>* h) {
  if (int rc = part_host_access(h, true)) return rc;
  const size_t E = h->E;
  h->be.memset(h->st.n_test, 0, E * 4);
  std::vector<int32_t> ph(E, PH_RESET);
  h->be.h2d(h->st.phase, ph.data(), E * 4);
  return h->be.sync() ? fail(h->be.error()) : 0;
}

template <class B>
int mark_exploit_done(Handle<B>* h) {
  if (int rc = part_host_access(h, true)) return rc;
  const size_t E = h->E;
  std::vector<uint32_t> fl(E);
  h->be.d2h(fl.data(), h->st.eflags, E * 4);
  for (auto& f : fl) f |= F_EXPLOIT_DONE;
  h->be.h2d(h->st.eflags, fl.data(), E * 4);
  if (h->be.sync()) return fail(h->be.error());
  return curve_exploit_sync(h);  // (no row was written for the rounds the flag now claims: they are not folded)
}

// Q-init patch rows (distr_q.py:81-181): the same rows for every env
template <class B>
int apply_qinit(Handle<B>* h, uint32_t n_rows, const uint32_t* row_port, const uint32_t* row_state,
                const double* values /*[n_rows][4], NaN = default_q*/) {
  if (n_rows == 0) return 0;
  uint32_t* d_port = h->template dalloc<uint32_t>(n_rows);
  uint32_t* d_state = h->template dalloc<uint32_t>(n_rows);
  double* d_vals = h->template dalloc<double>((size_t)n_rows * 4);
  if (!d_port || !d_state || !d_vals) return fail("sfl_apply_qinit: allocation failed");
  h->be.h2d(d_port, row_port, n_rows * 4);
  h->be.h2d(d_state, row_state, n_rows * 4);
  h->be.h2d(d_vals, values, (size_t)n_rows * 4 * 8);
  h->be.qinit(h->map, h->st, n_rows, d_port, d_state, d_vals);
  int rc = h->be.sync();
  // release the scratch
  for (int k = 0; k < 3; ++k) {
    h->be.free(h->allocs.back());
    h->allocs.pop_back();
  }
  return rc ? fail(h->be.error()) : 0;
}

// per-launch totals: one device reduction and a 32-byte copy instead of per-env arrays
template <class B>
int reduce_launch(Handle<B>* h) {
  uint64_t out[4] = {0, 0, 0, 0};
  h->be.reduce_launch(h->d_launch_dec, h->d_launch_ticks, h->d_launch_bytes, h->st.err, h->E, h->d_sums);
  h->be.d2h(out, h->d_sums, sizeof out);
  if (h->be.sync()) return fail(h->be.error());
  h->last_dec = out[0];
  h->last_ticks = out[1];
  h->last_bytes = out[2];
  h->last_err = (uint32_t)out[3];
  h->total_dec += out[0];
  return 0;
}

// the per-env error flags, when the launch totals reported any (h->last_err)
// before the host reads (write = false) or writes (true) the per-env scalars of a partitioned handle: the
// wave kernels' blocks copied back into the SflState arrays if they are newer; after a write the next
// part_local copies the arrays into the blocks again
template <class B>
int part_host_access(Handle<B>* h, bool write) {
  if (!h->part.world || !h->part.eblk) return 0;
  if (h->eblk_state == 1) {
    h->be.part_eblk(h->st, h->part, 1);
    if (h->be.sync()) return fail(h->be.error());
    h->eblk_state = 2;
  }
  if (write) h->eblk_state = 0;
  return 0;
}

template <class B>
int scan_errors(Handle<B>* h) {
  if (!h->last_err) return 0;
  if (int rc = part_host_access(h, false)) return rc;
  std::vector<uint32_t> err(h->E);
  h->be.d2h(err.data(), h->st.err, h->E * 4);
  if (h->be.sync()) return fail(h->be.error());
  for (uint32_t e = 0; e < h->E; ++e)
    if (err[e]) {
      char buf[256];
      snprintf(buf, sizeof buf, "env %u: error flags 0x%x (1=inf distance, 2=plan overflow, 4=port mismatch, 8=bad action, "
               "16=message segment overflow, 32=decayed lr beyond the ntab table: raise ntab)",
               e, err[e]);
      return fail(buf);
    }
  return 0;
}

template <class B>
int check_errors(Handle<B>* h) {
  if (int rc = reduce_launch(h)) return rc;
  return scan_errors(h);
}

template <class B>
int run(Handle<B>* h, const SflCtl& c_in, sfl_run_args* args) {
  if (h->bank.on) return fail("sfl_run: an evaluation handle has no per-env table (sfl_create_eval); drive it with sfl_bank_eval");
  if (h->part.world) return fail("sfl_run: the handle is graph-partitioned; drive it with sfl_part_*");
  if (h->env_mode) return fail("sfl_run: the handle is in external-action mode (sfl_env_begin); drive it with sfl_env_step");
  // (the grouped kernels are built plain only: no traced and no phase-timed instantiation)
  // (nor the kernels of a handle with a seed schedule)
  const bool grouped = h->map.env_group != nullptr || h->map.seed_sched != 0;
  if (grouped && args && args->trace && args->trace_cap > 0)
    return fail(h->map.env_group ? "sfl_run: a per-decision trace is not available on a handle with hyperparameter groups"
                                 : "sfl_run: a per-decision trace is not available on a handle with a seed schedule");
  SflCtl c = c_in;
  const size_t E = h->E, T = h->map.T;
  const int32_t cap = args ? args->stats_cap : 0;
  std::vector<void*> scratch;
  auto scr = [&](size_t bytes) -> void* {
    void* p = h->be.alloc(bytes ? bytes : 1);
    scratch.push_back(p);
    return p;
  };
  c.stats_cap = cap;
  c.stats_base = c_in.stats_base;
  if (args && cap > 0) {
    c.st_cum = (double*)scr((size_t)cap * E * 8);
    c.st_arrived = (int32_t*)scr((size_t)cap * E * 4);
    c.st_mf = (int32_t*)scr((size_t)cap * E * 4);
    c.st_dec = (int32_t*)scr((size_t)cap * E * 4);
    c.st_ticks = (int32_t*)scr((size_t)cap * E * 4);
    c.st_delays = (int32_t*)scr((size_t)cap * T * E * 4);
    c.sx_cum = (double*)scr((size_t)cap * E * 8);
    c.sx_arrived = (int32_t*)scr((size_t)cap * E * 4);
    for (void* p : scratch)
      if (!p) {
        for (void* q : scratch) h->be.free(q);
        return fail("sfl_run: stats allocation failed");
      }
    h->be.memset(c.sx_cum, 0, (size_t)cap * E * 8);
    h->be.memset(c.sx_arrived, 0, (size_t)cap * E * 4);
  }
  // sfl_step on a handle with a curve: the episode-end rows go to the handle's ring (row = episode index % ring_cap),
  // folded behind the launch; sfl_learn / sfl_test (args) keep their own buffers
  const bool curve = !args && h->cv.on;
  if (curve) {
    const CurveArgs& a = h->cv.a;
    c.stats_cap = a.ring_cap;
    c.stats_base = 0;
    c.st_cum = const_cast<double*>(a.st_cum);
    c.st_arrived = const_cast<int32_t*>(a.st_arrived);
    c.st_mf = const_cast<int32_t*>(a.st_mf);
    c.st_dec = const_cast<int32_t*>(a.st_dec);
    c.st_ticks = const_cast<int32_t*>(a.st_ticks);
    c.st_delays = const_cast<int32_t*>(a.st_delays);
  }
  // ... and with an exploit record the greedy rounds' rows too (c.exploit_freq: sfl_step's, the record's frequency)
  const bool xfold = curve && h->cv.x_on;
  if (xfold) {
    c.sx_cum = const_cast<double*>(h->cv.xa.sx_cum);
    c.sx_arrived = const_cast<int32_t*>(h->cv.xa.sx_arrived);
  }
  c.launch_dec = h->d_launch_dec;
  c.launch_ticks = h->d_launch_ticks;
  c.launch_bytes = h->d_launch_bytes;
  c.phase_cyc = args && !grouped ? h->d_phase : nullptr;  // learn / test (not the benchmark's sfl_step): phase timers
  uint64_t* d_trace = nullptr;
  uint64_t* d_trace_n = nullptr;
  if (args && args->trace && args->trace_cap > 0) {
    d_trace = (uint64_t*)scr((size_t)args->trace_cap * 32);
    d_trace_n = (uint64_t*)scr(8);
    if (!d_trace || !d_trace_n) {
      for (void* q : scratch) h->be.free(q);
      return fail("sfl_run: trace allocation failed");
    }
    h->be.memset(d_trace_n, 0, 8);
    c.trace = d_trace;
    c.trace_n = d_trace_n;
    c.trace_env = args->trace_env;
    c.trace_cap = args->trace_cap;
  }
  float ms = 0.f;
  int rc = h->be.run(h->map, h->st, c, h->variant, &ms);
  h->last_kernel_ms = ms;
  if (!rc && curve) rc = h->be.curve(h->cv.a, false);  // (timed on its own: elapsed_ms after the sync below)
  if (!rc && xfold) rc = h->be.curve_exploit(h->cv.xa, false);  // (likewise: elapsed_exploit_ms)
  if (!rc && args && cap > 0) {
    if (args->cum_reward) h->be.d2h(args->cum_reward, c.st_cum, (size_t)cap * E * 8);
    if (args->arrived) h->be.d2h(args->arrived, c.st_arrived, (size_t)cap * E * 4);
    if (args->malfunctions) h->be.d2h(args->malfunctions, c.st_mf, (size_t)cap * E * 4);
    if (args->decisions) h->be.d2h(args->decisions, c.st_dec, (size_t)cap * E * 4);
    if (args->ticks) h->be.d2h(args->ticks, c.st_ticks, (size_t)cap * E * 4);
    if (args->delays) h->be.d2h(args->delays, c.st_delays, (size_t)cap * T * E * 4);
    if (args->exploit_cum) h->be.d2h(args->exploit_cum, c.sx_cum, (size_t)cap * E * 8);
    if (args->exploit_arrived) h->be.d2h(args->exploit_arrived, c.sx_arrived, (size_t)cap * E * 4);
  }
  if (!rc && d_trace) {
    h->be.d2h(args->trace_n, d_trace_n, 8);
    h->be.d2h(args->trace, d_trace, (size_t)args->trace_cap * 32);
  }
  if (!rc) rc = h->be.sync();
  for (void* p : scratch) h->be.free(p);
  if (rc) return fail(std::string("sfl_run: ") + h->be.error());
  if (curve) {
    h->cv.last_ms = h->be.elapsed_ms();
    h->cv.x_last_ms = xfold ? h->be.elapsed_exploit_ms() : 0.f;
    h->cv.last_ms += h->cv.x_last_ms;
    h->cv.total_ms += h->cv.last_ms;
    h->cv.x_total_ms += h->cv.x_last_ms;
  }
  return check_errors(h);
}

// ---------------------------------------------------------------------------
// policy-bank evaluation (include/sfl.h sfl_create_eval / sfl_bank_*; sfl_eval.h)
// ---------------------------------------------------------------------------
template <class B>
int bank_check(Handle<B>* h, const char* fn, uint32_t p) {
  if (!h->bank.on) return fail(std::string(fn) + ": not an evaluation handle (sfl_create_eval)");
  if (p >= h->bank.P) return fail(std::string(fn) + ": policy " + std::to_string(p) + " of " + std::to_string(h->bank.P));
  return 0;
}

template <class B>
int bank_set(Handle<B>* h, uint32_t p, const double* q, const uint32_t* touched) {
  if (int rc = bank_check(h, "sfl_bank_set", p)) return rc;
  const SflMap& m = h->map;
  if (q) h->be.h2d(h->bank.q + (size_t)p * m.lrn.q_per_env, q, m.lrn.q_per_env * 8);
  if (touched) h->be.h2d(h->bank.keys + (size_t)p * m.lrn.touched_words, touched, (size_t)m.lrn.touched_words * 4);
  if (h->be.sync()) return fail(h->be.error());
  h->bank.set[p] = 1;
  return 0;
}

template <class B>
int bank_get(Handle<B>* h, uint32_t p, double* q, uint32_t* touched) {
  if (int rc = bank_check(h, "sfl_bank_get", p)) return rc;
  const SflMap& m = h->map;
  if (q) h->be.d2h(q, h->bank.q + (size_t)p * m.lrn.q_per_env, m.lrn.q_per_env * 8);
  if (touched) h->be.d2h(touched, h->bank.keys + (size_t)p * m.lrn.touched_words, (size_t)m.lrn.touched_words * 4);
  return h->be.sync() ? fail(h->be.error()) : 0;
}

// device to device, from a training handle on the same device (its calls are synchronous: nothing of it is in flight)
template <class B>
int bank_copy(Handle<B>* h, uint32_t p, Handle<B>* src, int32_t kind, uint32_t index) {
  if (int rc = bank_check(h, "sfl_bank_copy", p)) return rc;
  if (!src) return fail("sfl_bank_copy: null source handle");
  if (src->bank.on) return fail("sfl_bank_copy: the source is itself an evaluation handle (use sfl_bank_get / sfl_bank_set)");
  if (src->part.world) return fail("sfl_bank_copy: the source is graph-partitioned (its tables are owned rows)");
  if (src->device != h->device)
    return fail("sfl_bank_copy: the source is on device " + std::to_string(src->device) + ", the bank on device " +
                std::to_string(h->device));
  const SflMap &m = h->map, &sm = src->map;
  if (sm.lrn.q_per_env != m.lrn.q_per_env || sm.rows_per_env != m.rows_per_env)
    return fail("sfl_bank_copy: the source's Q layout differs (q_per_env " + std::to_string(sm.lrn.q_per_env) + " / " +
                std::to_string(m.lrn.q_per_env) + ", rows_per_env " + std::to_string(sm.rows_per_env) + " / " +
                std::to_string(m.rows_per_env) + "): another map");
  if (memcmp(&sm.dec.default_q, &m.dec.default_q, 8) != 0) return fail("sfl_bank_copy: the source's default_q differs");
  const double* q = nullptr;
  const uint32_t* keys = nullptr;
  if (kind == SFL_BANK_FROM_ENV) {
    if (index >= src->E) return fail("sfl_bank_copy: env " + std::to_string(index) + " of " + std::to_string(src->E));
    q = src->st.lrn.q + (size_t)index * m.lrn.q_per_env;
    keys = src->st.lrn.touched + (size_t)index * m.lrn.touched_words;
  } else if (kind == SFL_BANK_FROM_COHORT) {
    if (index >= src->cons_n)
      return fail("sfl_bank_copy: no consensus cohort " + std::to_string(index) + " (the source's last sfl_consensus made " +
                  std::to_string(src->cons_n) + ")");
    q = src->cons_q + (size_t)index * m.lrn.q_per_env;
    keys = src->cons_keys + (size_t)index * m.lrn.touched_words;
  } else {
    return fail("sfl_bank_copy: kind " + std::to_string(kind) + " (SFL_BANK_FROM_ENV or SFL_BANK_FROM_COHORT)");
  }
  h->be.d2d(h->bank.q + (size_t)p * m.lrn.q_per_env, q, m.lrn.q_per_env * 8);
  h->be.d2d(h->bank.keys + (size_t)p * m.lrn.touched_words, keys, (size_t)m.lrn.touched_words * 4);
  if (h->be.sync()) return fail(std::string("sfl_bank_copy: ") + h->be.error());
  h->bank.set[p] = 1;
  return 0;
}

// one greedy episode per env from a reset (sfl_test's start and end: n_test 0, every env at PH_RESET before and
// after), env e on table env_policy[e]; the fold behind the launch; the optional per-env outputs
template <class B>
int bank_eval(Handle<B>* h, const uint32_t* env_policy, sfl_eval_out* out) {
  typename Handle<B>::Bank& bk = h->bank;
  if (!bk.on) return fail("sfl_bank_eval: not an evaluation handle (sfl_create_eval)");
  if (!env_policy) return fail("sfl_bank_eval: null env_policy");
  const size_t E = h->E, T = h->map.T;
  for (size_t e = 0; e < E; ++e) {
    if (env_policy[e] >= bk.P)
      return fail("sfl_bank_eval: env " + std::to_string(e) + " follows policy " + std::to_string(env_policy[e]) + " of " +
                  std::to_string(bk.P));
    if (!bk.set[env_policy[e]])
      return fail("sfl_bank_eval: env " + std::to_string(e) + " follows policy " + std::to_string(env_policy[e]) +
                  ", which was never set (sfl_bank_set / sfl_bank_copy)");
  }
  h->be.h2d(bk.policy, env_policy, E * 4);
  if (int rc = test_begin(h)) return rc;  // (synchronises: env_policy is the caller's memory)
  SflCtl c{};
  c.mode = MODE_BANK;
  c.ep_target = 1;
  c.stats_cap = 1;
  c.st_cum = bk.cum;
  c.st_arrived = bk.arrived;
  c.st_mf = bk.mf;
  c.st_dec = bk.dec;
  c.st_ticks = bk.ticks;
  c.st_delays = bk.delays;
  c.ev_at_dest = bk.at_dest;
  c.ev_trunc = bk.trunc;
  c.ev_last_move = bk.last_move;
  if (bk.rec_n) {
    c.rec_slot = bk.rec_slot;
    c.rec_cell = bk.rec_cell;
    c.rec_bits = bk.rec_bits;
    c.rec_dec = bk.rec_rows;
    c.rec_tick_cap = bk.rec_tick_cap;
    c.rec_dec_cap = bk.rec_dec_cap;
  }
  c.launch_dec = h->d_launch_dec;
  c.launch_ticks = h->d_launch_ticks;
  c.launch_bytes = h->d_launch_bytes;
  float ms = 0.f;
  bk.folded = false;
  bk.diagnosed = false;
  bk.recorded = false;
  int rc = h->be.run(h->map, h->st, c, h->variant, &ms);
  h->last_kernel_ms = ms;
  EvalArgs a{};
  a.E = h->E;
  a.n_policies = bk.P;
  a.T = h->map.T;
  a.policy = bk.policy;
  a.cum = bk.cum;
  a.arrived = bk.arrived;
  a.mf = bk.mf;
  a.dec = bk.dec;
  a.ticks = bk.ticks;
  a.trunc = bk.trunc;
  a.delays = bk.delays;
  a.at_dest = bk.at_dest;
  a.cells = bk.cells;
  if (!rc) rc = h->be.eval_fold(a);  // (timed on its own: elapsed_ms after the sync below)
  if (!rc && out) {
    if (out->cum_reward) h->be.d2h_async(out->cum_reward, bk.cum, E * 8);
    if (out->arrived) h->be.d2h_async(out->arrived, bk.arrived, E * 4);
    if (out->malfunctions) h->be.d2h_async(out->malfunctions, bk.mf, E * 4);
    if (out->decisions) h->be.d2h_async(out->decisions, bk.dec, E * 4);
    if (out->ticks) h->be.d2h_async(out->ticks, bk.ticks, E * 4);
    if (out->truncated) h->be.d2h_async(out->truncated, bk.trunc, E * 4);
    if (out->delays) h->be.d2h_async(out->delays, bk.delays, T * E * 4);
    if (out->at_dest) h->be.d2h_async(out->at_dest, bk.at_dest, T * E);
  }
  if (!rc) {  // leave the envs ready for a fresh episode, as sfl_test does
    std::vector<int32_t> ph(E, PH_RESET);
    h->be.h2d(h->st.phase, ph.data(), E * 4);
    rc = h->be.sync();
  }
  if (rc) return fail(std::string("sfl_bank_eval: ") + h->be.error());
  bk.last_ms = h->be.elapsed_ms();
  bk.total_ms += bk.last_ms;
  if (int rc2 = check_errors(h)) return rc2;
  bk.folded = true;
  bk.recorded = bk.rec_n != 0;
  return 0;
}

template <class B>
int bank_read(Handle<B>* h, sfl_eval_cell* out) {
  if (!h->bank.on) return fail("sfl_bank_read: not an evaluation handle (sfl_create_eval)");
  if (!out) return fail("sfl_bank_read: null argument");
  if (!h->bank.folded) return fail("sfl_bank_read: no successful sfl_bank_eval yet");
  h->be.d2h(out, h->bank.cells, (size_t)h->bank.P * EV_WORDS * 8);
  return h->be.sync() ? fail(h->be.error()) : 0;
}

// the non-arrival diagnosis of the last sfl_bank_eval (include/sfl.h sfl_bank_diag*; sfl_diag.h): the classify pass and
// the fold queued on the handle's stream, the optional per-train outputs behind them
template <class B>
int bank_diag(Handle<B>* h, int32_t stall, sfl_diag_out* out) {
  typename Handle<B>::Bank& bk = h->bank;
  if (!bk.on) return fail("sfl_bank_diag: not an evaluation handle (sfl_create_eval)");
  if (!bk.folded) return fail("sfl_bank_diag: no successful sfl_bank_eval yet");
  if (stall < 1) return fail("sfl_bank_diag: stall " + std::to_string(stall) + " (the window is at least 1 tick)");
  const size_t E = h->E, T = h->map.T;
  DiagArgs a{};
  a.E = h->E;
  a.n_policies = bk.P;
  a.HW = (uint32_t)h->map.HW;
  a.T = h->map.T;
  a.stall = stall;
  a.wave = h->variant > 0 ? 1 : 0;
  a.policy = bk.policy;
  a.ticks = bk.ticks;
  a.trunc = bk.trunc;
  a.last_move = bk.last_move;
  a.tr_pos = h->st.tr_pos;
  a.tr_bits = h->st.tr_bits;
  a.move_tab = h->map.move_tab;
  a.cls = bk.dg_cls;
  a.blocker = bk.dg_blocker;
  a.stalled_for = bk.dg_sf;
  a.env_aux = bk.dg_aux;
  a.hot = bk.dg_hot;
  a.cells = bk.dg_cells;
  bk.diagnosed = false;
  int rc = h->be.diag(a);  // (timed on its own: elapsed_ms after the sync below)
  if (!rc && out) {
    if (out->cls) h->be.d2h_async(out->cls, bk.dg_cls, T * E);
    if (out->blocker) h->be.d2h_async(out->blocker, bk.dg_blocker, T * E * 2);
    if (out->stalled_for) h->be.d2h_async(out->stalled_for, bk.dg_sf, T * E * 4);
  }
  if (!rc) rc = h->be.sync();
  if (rc) return fail(std::string("sfl_bank_diag: ") + h->be.error());
  bk.dg_last_ms = h->be.elapsed_ms();
  bk.dg_total_ms += bk.dg_last_ms;
  bk.diagnosed = true;
  return 0;
}

template <class B>
int bank_diag_read(Handle<B>* h, sfl_diag_cell* out) {
  if (!h->bank.on) return fail("sfl_bank_diag_read: not an evaluation handle (sfl_create_eval)");
  if (!out) return fail("sfl_bank_diag_read: null argument");
  if (!h->bank.folded) return fail("sfl_bank_diag_read: no successful sfl_bank_eval yet");
  if (!h->bank.diagnosed) return fail("sfl_bank_diag_read: no successful sfl_bank_diag of the last evaluation yet");
  h->be.d2h(out, h->bank.dg_cells, (size_t)h->bank.P * DG_WORDS * 8);
  return h->be.sync() ? fail(h->be.error()) : 0;
}

template <class B>
int bank_diag_hot(Handle<B>* h, uint32_t p, uint32_t* out) {
  if (int rc = bank_check(h, "sfl_bank_diag_hot", p)) return rc;
  if (!out) return fail("sfl_bank_diag_hot: null argument");
  if (!h->bank.folded) return fail("sfl_bank_diag_hot: no successful sfl_bank_eval yet");
  if (!h->bank.diagnosed) return fail("sfl_bank_diag_hot: no successful sfl_bank_diag of the last evaluation yet");
  const size_t HW = (size_t)h->map.HW;
  h->be.d2h(out, h->bank.dg_hot + (size_t)p * HW, HW * 4);
  return h->be.sync() ? fail(h->be.error()) : 0;
}

// the recording of listed envs' episodes (include/sfl.h sfl_bank_record*; sfl_rec.h): arming allocates
// the buffers and uploads the per-env slot index, the episode launch of every later sfl_bank_eval fills them, the
// readers copy a slot back and the traffic fold reduces the slots of one policy -- all on the handle's stream
static_assert(REC_DEC_WORDS == SFL_REC_DEC_WORDS && REC_NOW == SFL_REC_NOW && REC_SWITCH == SFL_REC_SWITCH &&
                  REC_TRAIN == SFL_REC_TRAIN && REC_SLOT == SFL_REC_SLOT && REC_STATE == SFL_REC_STATE &&
                  REC_MASK == SFL_REC_MASK && REC_ACTION == SFL_REC_ACTION && REC_REWARD == SFL_REC_REWARD &&
                  REC_NEXT_SWITCH == SFL_REC_NEXT_SWITCH && REC_STEP_NOW == SFL_REC_STEP_NOW,
              "a recorded decision's row: the kernels' word order is the header's");
template <class B>
void bank_record_free(Handle<B>* h) {
  typename Handle<B>::Bank& bk = h->bank;
  for (void* p : {(void*)bk.rec_env_d, (void*)bk.rec_slot, (void*)bk.rec_cell, (void*)bk.rec_bits, (void*)bk.rec_rows})
    if (p) h->dfree(p);
  bk.rec_env_d = nullptr;
  bk.rec_slot = nullptr;
  bk.rec_cell = nullptr;
  bk.rec_bits = nullptr;
  bk.rec_rows = nullptr;
  bk.rec_n = 0;
  bk.rec_tick_cap = bk.rec_dec_cap = 0;
  bk.rec_env.clear();
  bk.recorded = false;
}

template <class B>
int bank_record(Handle<B>* h, uint32_t n, const uint32_t* envs, int32_t tick_cap, int32_t dec_cap) {
  typename Handle<B>::Bank& bk = h->bank;
  if (!bk.on) return fail("sfl_bank_record: not an evaluation handle (sfl_create_eval)");
  if (n == 0) {  // disarm
    if (h->be.sync()) return fail(std::string("sfl_bank_record: ") + h->be.error());
    bank_record_free(h);
    return 0;
  }
  if (!envs) return fail("sfl_bank_record: null envs");
  if (tick_cap < 1) return fail("sfl_bank_record: tick_cap " + std::to_string(tick_cap) + " (at least 1)");
  if (dec_cap < 1) return fail("sfl_bank_record: dec_cap " + std::to_string(dec_cap) + " (at least 1)");
  const size_t E = h->E, T = h->map.T;
  if (n > E) return fail("sfl_bank_record: " + std::to_string(n) + " envs listed of " + std::to_string(E) + " (distinct envs only)");
  std::vector<int32_t> slot(E, -1);
  for (uint32_t k = 0; k < n; ++k) {
    if (envs[k] >= E) return fail("sfl_bank_record: env " + std::to_string(envs[k]) + " of " + std::to_string(E));
    if (slot[envs[k]] >= 0) return fail("sfl_bank_record: env " + std::to_string(envs[k]) + " is listed twice");
    slot[envs[k]] = (int32_t)k;
  }
  // n * (tick_cap * T * 8 + dec_cap * 4 * SFL_REC_DEC_WORDS) bytes, in 128 bits: the caps are up to 2^31 - 1
  const unsigned __int128 per = (unsigned __int128)(uint32_t)tick_cap * T * 8u + (unsigned __int128)(uint32_t)dec_cap * 4u * SFL_REC_DEC_WORDS;
  if (per * n > (unsigned __int128)SFL_REC_MAX_BYTES)
    return fail("sfl_bank_record: " + std::to_string(n) + " envs x (" + std::to_string(tick_cap) + " ticks x " + std::to_string(T) +
                " trains x 8 + " + std::to_string(dec_cap) + " decisions x " + std::to_string(4 * SFL_REC_DEC_WORDS) +
                ") bytes exceed SFL_REC_MAX_BYTES");
  if (h->be.sync()) return fail(std::string("sfl_bank_record: ") + h->be.error());
  bank_record_free(h);  // (an armed recording is replaced)
  const size_t nf = (size_t)n * (size_t)tick_cap * T, nr = (size_t)n * (size_t)dec_cap * SFL_REC_DEC_WORDS;
  bk.rec_env_d = h->template dalloc<uint32_t>(n);
  bk.rec_slot = h->template dalloc<int32_t>(E);
  bk.rec_cell = h->template dalloc<int32_t>(nf);
  bk.rec_bits = h->template dalloc<uint32_t>(nf);
  bk.rec_rows = h->template dalloc<int32_t>(nr);
  if (!bk.rec_env_d || !bk.rec_slot || !bk.rec_cell || !bk.rec_bits || !bk.rec_rows) {
    bank_record_free(h);
    return fail("sfl_bank_record: device allocation failed");
  }
  h->be.h2d(bk.rec_env_d, envs, (size_t)n * 4);
  h->be.h2d(bk.rec_slot, slot.data(), E * 4);
  h->be.memset(bk.rec_cell, 0xFF, nf * 4);  // (words past the kept frames / rows: off the map, -1)
  h->be.memset(bk.rec_bits, 0, nf * 4);
  h->be.memset(bk.rec_rows, 0xFF, nr * 4);
  if (h->be.sync()) {  // (synchronises: envs and slot are host memory)
    bank_record_free(h);
    return fail(std::string("sfl_bank_record: ") + h->be.error());
  }
  bk.rec_n = n;
  bk.rec_tick_cap = tick_cap;
  bk.rec_dec_cap = dec_cap;
  bk.rec_env.assign(envs, envs + n);
  return 0;
}

template <class B>
int bank_record_info(Handle<B>* h, sfl_record_info* out) {
  if (!h->bank.on) return fail("sfl_bank_record_info: not an evaluation handle (sfl_create_eval)");
  if (!out) return fail("sfl_bank_record_info: null argument");
  out->n = h->bank.rec_n;
  out->tick_cap = h->bank.rec_tick_cap;
  out->dec_cap = h->bank.rec_dec_cap;
  out->dec_words = SFL_REC_DEC_WORDS;
  return 0;
}

// what every reader asks first: an evaluation handle with a recording armed and an evaluation behind the arming
template <class B>
int bank_record_check(Handle<B>* h, const char* fn) {
  if (!h->bank.on) return fail(std::string(fn) + ": not an evaluation handle (sfl_create_eval)");
  if (!h->bank.rec_n) return fail(std::string(fn) + ": no recording armed (sfl_bank_record)");
  if (!h->bank.recorded) return fail(std::string(fn) + ": no successful sfl_bank_eval since the recording was armed");
  return 0;
}

template <class B>
int bank_record_counts(Handle<B>* h, int32_t* ticks, int32_t* decisions) {
  if (int rc = bank_record_check(h, "sfl_bank_record_counts")) return rc;
  typename Handle<B>::Bank& bk = h->bank;
  // the evaluation's own per-env outputs, copied whole (one copy each) and indexed at the listed envs on the host
  std::vector<int32_t> t(ticks ? h->E : 0), d(decisions ? h->E : 0);
  if (ticks) h->be.d2h_async(t.data(), bk.ticks, (size_t)h->E * 4);
  if (decisions) h->be.d2h_async(d.data(), bk.dec, (size_t)h->E * 4);
  if (h->be.sync()) return fail(h->be.error());
  for (uint32_t k = 0; k < bk.rec_n; ++k) {
    if (ticks) ticks[k] = t[bk.rec_env[k]];
    if (decisions) decisions[k] = d[bk.rec_env[k]];
  }
  return 0;
}

template <class B>
int bank_record_read(Handle<B>* h, uint32_t k, int32_t* cell, uint32_t* bits, int32_t* dec) {
  if (int rc = bank_record_check(h, "sfl_bank_record_read")) return rc;
  typename Handle<B>::Bank& bk = h->bank;
  if (k >= bk.rec_n) return fail("sfl_bank_record_read: slot " + std::to_string(k) + " of " + std::to_string(bk.rec_n));
  const size_t nf = (size_t)bk.rec_tick_cap * (size_t)h->map.T, nr = (size_t)bk.rec_dec_cap * SFL_REC_DEC_WORDS;
  if (cell) h->be.d2h_async(cell, bk.rec_cell + (size_t)k * nf, nf * 4);
  if (bits) h->be.d2h_async(bits, bk.rec_bits + (size_t)k * nf, nf * 4);
  if (dec) h->be.d2h_async(dec, bk.rec_rows + (size_t)k * nr, nr * 4);
  return h->be.sync() ? fail(h->be.error()) : 0;
}

template <class B>
int bank_record_traffic(Handle<B>* h, uint32_t p, sfl_record_traffic* out) {
  if (int rc = bank_record_check(h, "sfl_bank_record_traffic")) return rc;
  typename Handle<B>::Bank& bk = h->bank;
  if (p >= bk.P) return fail("sfl_bank_record_traffic: policy " + std::to_string(p) + " of " + std::to_string(bk.P));
  if (!out) return fail("sfl_bank_record_traffic: null argument");
  const size_t HW = (size_t)h->map.HW, S = (size_t)h->map.lrn.S;
  RecArgs a{};
  a.n = bk.rec_n;
  a.E = h->E;
  a.HW = (uint32_t)HW;
  a.S = (uint32_t)S;
  a.T = h->map.T;
  a.tick_cap = bk.rec_tick_cap;
  a.dec_cap = bk.rec_dec_cap;
  a.p = p;
  a.env = bk.rec_env_d;
  a.policy = bk.policy;
  a.ticks = bk.ticks;
  a.dec = bk.dec;
  a.cell = bk.rec_cell;
  a.bits = bk.rec_bits;
  a.rows = bk.rec_rows;
  a.sw_na = h->map.sw_na;
  a.out = bk.rec_out;
  int rc = h->be.rec_traffic(a);  // (timed on its own: elapsed_ms after the sync below)
  if (!rc) {
    if (out->occupancy) h->be.d2h_async(out->occupancy, bk.rec_out, HW * 4);
    if (out->standing) h->be.d2h_async(out->standing, bk.rec_out + HW, HW * 4);
    if (out->standing_malfunction) h->be.d2h_async(out->standing_malfunction, bk.rec_out + 2 * HW, HW * 4);
    if (out->decisions) h->be.d2h_async(out->decisions, bk.rec_out + 3 * HW, S * 4);
    if (out->stops) h->be.d2h_async(out->stops, bk.rec_out + 3 * HW + S, S * 4);
    rc = h->be.sync();
  }
  if (rc) return fail(std::string("sfl_bank_record_traffic: ") + h->be.error());
  bk.rc_last_ms = h->be.elapsed_ms();
  bk.rc_total_ms += bk.rc_last_ms;
  return 0;
}

// ---------------------------------------------------------------------------
// external-action mode (include/sfl.h sfl_env_begin / sfl_env_step; SflExt in sfl_core.h)
// ---------------------------------------------------------------------------
// the row of external-action mode's wave kernel for a handle created on row v: v itself, but for the LM row its twin
// without the LDS map tables (copying 64 KB of tables per block buys nothing for one decision per launch)
inline int ext_variant(int v) {
  if (v <= 0 || !kVariants[v].LM) return v;
  for (int u = 1; u < kNumVariants; ++u) {
    const WaveShape &a = kVariants[u], &b = kVariants[v];
    if (!a.LM && a.PPL == b.PPL && a.SPL == b.SPL && a.TW == b.TW && a.G == b.G) return u;
  }
  return 0;
}

// ---------------------------------------------------------------------------
// external-action mode's transition assembler (include/sfl.h sfl_env_trans_*; sfl_trans.h)
// ---------------------------------------------------------------------------
template <class B>
int trans_begin(Handle<B>* h, const sfl_env_trans_io* io) {
  const char* fn = "sfl_env_trans_begin: ";
  if (h->bank.on) return fail(std::string(fn) + "an evaluation handle has no external-action mode (sfl_create_eval)");
  if (h->part.world) return fail(std::string(fn) + "the handle is graph-partitioned");
  if (!h->env_mode) return fail(std::string(fn) + "the handle is not in external-action mode (call sfl_env_begin first)");
  if (!io) return fail(std::string(fn) + "null argument");
  if (io->capacity == 0) return fail(std::string(fn) + "capacity must be at least 1");
  if (io->capacity > 0x7FFFFFFFu) return fail(std::string(fn) + "capacity above 2^31 - 1");
  if (!io->env || !io->train || !io->now || !io->agent || !io->action || !io->reward || !io->next_agent ||
      !io->next_n_actions || !io->terminal || !io->total || !io->last_count || !io->dropped)
    return fail(std::string(fn) + "null column (only obs, next_obs and next_action_mask may be null)");
  if (io->next_action_mask && h->max_na > SFL_MAX_ACTIONS)
    return fail(std::string(fn) + "the map has a switch with more than SFL_MAX_ACTIONS actions (the dense action mask "
                "cannot hold it)");
  if (((uintptr_t)io->obs & 7u) || ((uintptr_t)io->next_obs & 7u) || ((uintptr_t)io->next_action_mask & 15u))
    return fail(std::string(fn) + "obs and next_obs must be 8-byte and next_action_mask 16-byte aligned");
  if (h->map.lrn.S > 0xFFFF) return fail(std::string(fn) + "more than 65,535 switches");
  const size_t E = h->E, T = h->map.T, S = h->map.lrn.S;
  const size_t nb = (E + TRANS_BLOCK - 1) / TRANS_BLOCK;
  TransArgs& a = h->tr.a;
  if (!a.tab) {
    a.tab = h->template dalloc<TransEntry>(E * T * S);
    a.latch = h->template dalloc<TransLatch>(E);
    a.live = h->template dalloc<uint32_t>(E);
    a.seen = h->template dalloc<uint32_t>(MAXW * E);
    a.epoch = h->template dalloc<uint32_t>(E);
    a.cnt = h->template dalloc<uint32_t>(E);
    a.blk = h->template dalloc<uint32_t>(nb);
    a.cur = h->template dalloc<uint64_t>(4);
    if (!a.tab || !a.latch || !a.live || !a.seen || !a.epoch || !a.cnt || !a.blk || !a.cur) {
      a.tab = nullptr;
      return fail(std::string(fn) + "allocation failed");
    }
  }
  a.E = h->E;
  a.N = io->capacity;
  a.S = h->map.lrn.S;
  a.T = h->map.T;
  a.K = h->map.dec.K;
  a.sw_np = h->map.sw_np;
  a.sw_na = h->map.sw_na;
  a.sw_rc = h->d_sw_rc;
  a.st_rc = h->d_st_rc;
  a.r_env = io->env;
  a.r_train = io->train;
  a.r_now = io->now;
  a.r_agent = io->agent;
  a.r_action = io->action;
  a.r_reward = io->reward;
  a.r_next_agent = io->next_agent;
  a.r_next_na = io->next_n_actions;
  a.r_terminal = io->terminal;
  a.r_obs = io->obs;
  a.r_next_obs = io->next_obs;
  a.r_next_mask = io->next_action_mask;
  a.total = io->total;
  a.last_count = io->last_count;
  a.dropped = io->dropped;
  // an empty table (no stamp is an episode count + 1), no decision latched (agent -1), the cursor and the caller's
  // counters at zero: memsets on the handle's stream, no wait
  h->be.memset(a.tab, 0, E * T * S * sizeof(TransEntry));
  h->be.memset(a.latch, 0xFF, E * sizeof(TransLatch));
  h->be.memset(a.live, 0, E * 4);
  h->be.memset(a.seen, 0, MAXW * E * 4);
  h->be.memset(a.epoch, 0, E * 4);
  h->be.memset(a.cur, 0, 4 * 8);
  h->be.memset(a.total, 0, 8);
  h->be.memset(a.last_count, 0, 4);
  h->be.memset(a.dropped, 0, E * 8);
  h->tr.parity = 0;
  h->tr.on = true;
  return 0;
}

template <class B>
int trans_end(Handle<B>* h) {
  if (!h->tr.on) return fail("sfl_env_trans_end: no transition assembler is running (sfl_env_trans_begin)");
  h->tr.on = false;
  return 0;
}

// behind every env step of the handle: the assembler on what this call's step read (the handle's action buffer) and
// wrote (x: the handle's own buffers, or the caller's of sfl_env_step_dev), queued on the same stream
template <class B>
int trans_after_step(Handle<B>* h, const SflExt& x) {
  if (!h->tr.on) return 0;
  TransArgs a = h->tr.a;
  a.parity = h->tr.parity;
  a.actions = h->ext.actions;
  a.agent = x.agent;
  a.train = x.train;
  a.slot = x.slot;
  a.state = x.state;
  a.mask = x.mask;
  a.reward = x.reward;
  a.now = x.now;
  a.next_sw = x.next_sw;
  a.arrived = x.arrived;
  if (h->be.trans(a)) return fail(std::string("sfl_env_trans: ") + h->be.error());
  h->tr.parity ^= 1u;
  return 0;
}

// wave: sfl_env_begin_wave -- the same fresh start on the wave shape the handle was created with (EXT in sfl_wave.h)
template <class B>
int env_begin(Handle<B>* h, bool wave = false) {
  const std::string fn = wave ? "sfl_env_begin_wave" : "sfl_env_begin";
  if (h->bank.on) return fail(fn + ": an evaluation handle runs sfl_bank_eval only (sfl_create_eval)");
  if (h->part.world) return fail(fn + ": the handle is graph-partitioned");
  if (h->map.env_group) return fail(fn + ": the handle has hyperparameter groups (sfl_set_hparam_groups)");
  if (h->map.seed_sched && (h->map.seed_flags & SEED_HELDOUT_EXPLOIT))
    return fail(fn + ": the handle's seed schedule has SFL_SEED_HELDOUT_EXPLOIT, and no episode of this mode is greedy");
  int variant = 0;
  if (wave) {
    if (!B::kHasWave)
      return fail(fn + ": this build has no wave kernels (the host build runs the lane-per-env body only)");
    variant = ext_variant(h->created_variant);
    if (variant <= 0)
      return fail(fn + ": the handle has no wave shape (" +
                  (h->variant_note.empty() ? std::string("SFL_KERNEL=scalar") : h->variant_note) + ")");
  }
  const size_t E = h->E, T = h->map.T, S = h->map.lrn.S, NP = h->map.NP;
  if (!h->d_ext) {
    SflExt& x = h->ext;
    x.actions = h->template dalloc<int32_t>(E);
    x.agent = h->template dalloc<int32_t>(E);
    x.train = h->template dalloc<int32_t>(E);
    x.slot = h->template dalloc<int32_t>(E);
    x.state = h->template dalloc<uint32_t>(E);
    x.mask = h->template dalloc<uint32_t>(E);
    x.reward = h->template dalloc<int32_t>(E);
    x.now = h->template dalloc<int32_t>(E);
    x.next_sw = h->template dalloc<int32_t>(E);
    x.step_now = h->template dalloc<int32_t>(E);
    x.arrived = h->template dalloc<uint32_t>(MAXW * E);
    x.n_mf = h->template dalloc<int32_t>(E);
    x.delays = h->template dalloc<int32_t>(T * E);
    x.truncated = h->template dalloc<int32_t>(E);
    h->d_ext = h->template dalloc<SflExt>(1);
    if (!x.actions || !x.agent || !x.train || !x.slot || !x.state || !x.mask || !x.reward || !x.now || !x.next_sw ||
        !x.step_now || !x.arrived || !x.n_mf || !x.delays || !x.truncated || !h->d_ext)
      return fail(fn + ": allocation failed");
    h->be.h2d(h->d_ext, &h->ext, sizeof(SflExt));
  }
  // a fresh env (a new ASyncSwitchEnv): the lane-per-env body and its state layout, or the wave shape and its
  // env-major one (the memsets below do not depend on the layout), every env at reset
  h->variant = variant;
  h->env_mode = true;
  h->tr.on = false;  // (either begin call ends a running transition assembler)
  SflState& st = h->st;
  std::vector<int32_t> ph(E, PH_RESET);
  h->be.h2d(st.phase, ph.data(), E * 4);
  h->be.memset(st.eflags, 0, E * 4);
  h->be.memset(st.elapsed, 0, E * 4);
  h->be.memset(st.epoch, 0, E * 4);
  h->be.memset(st.err, 0, E * 4);
  h->be.memset(st.masks, 0, 4 * MAXW * E * 4);
  h->be.memset(st.tr_pos, 0xFF, T * E * 4);
  h->be.memset(st.tr_bits, 0, T * E * 4);
  h->be.memset(st.tr_plan, 0, T * E * 4);
  h->be.memset(st.tr_next, 0, T * E * 2);
  h->be.memset(st.tr_prev, 0xFF, T * E * 2);
  h->be.memset(st.tr_src, 0xFF, T * E * 2);
  h->be.memset(st.tr_dec, 0, T * E * 2);
  h->be.memset(st.own_n, 0, T * E);
  h->be.memset(st.occ, 0xFF, (size_t)h->map.HW * E);
  h->be.memset(st.claim, 0xFF, (size_t)h->map.HW * E);
  h->be.memset(st.sem, 0, NP * E * 8);
  h->be.memset(st.lrn.slot, 0, S * T * E * 8);
  h->be.memset(st.step_ctr, 0, E * 8);
  // a seed schedule counts the episodes an env has started since here, minus one, in ep_t
  if (h->map.seed_sched) {
    h->be.memset(st.ep_t, 0xFF, E * 4);
    h->be.h2d(st.ep_seed, h->seeds.data(), E * 8);  // (the base seed before the first reset)
  }
  std::vector<int32_t> none(E, -1);
  h->be.h2d((void*)h->ext.actions, none.data(), E * 4);
  return h->be.sync() ? fail(h->be.error()) : 0;
}

template <class B>
int env_step(Handle<B>* h, sfl_env_io* io) {
  if (!h->env_mode) return fail("sfl_env_step: call sfl_env_begin first");
  if (!io || !io->agent) return fail("sfl_env_step: null argument");
  const size_t E = h->E, T = h->map.T;
  const SflExt& x = h->ext;
  if (io->actions) h->be.h2d((void*)x.actions, io->actions, E * 4);
  else h->be.memset((void*)x.actions, 0xFF, E * 4);
  SflCtl c{};
  c.mode = 2;
  c.ext = h->d_ext;
  c.launch_dec = h->d_launch_dec;
  c.launch_ticks = h->d_launch_ticks;
  c.launch_bytes = h->d_launch_bytes;
  float ms = 0.f;
  if (h->be.run_ext(h->map, h->st, c, h->variant, &ms)) return fail(std::string("sfl_env_step: ") + h->be.error());
  h->last_kernel_ms = ms;
  if (int rc = trans_after_step(h, x)) return rc;
  auto get = [&](void* dst, const void* src, size_t n) {
    if (dst) h->be.d2h_async(dst, src, n);
  };
  get(io->agent, x.agent, E * 4);
  get(io->train, x.train, E * 4);
  get(io->slot, x.slot, E * 4);
  get(io->state, x.state, E * 4);
  get(io->mask, x.mask, E * 4);
  get(io->reward, x.reward, E * 4);
  get(io->now, x.now, E * 4);
  get(io->next_switch, x.next_sw, E * 4);
  get(io->step_now, x.step_now, E * 4);
  get(io->arrived, x.arrived, MAXW * E * 4);
  get(io->malfunctions, x.n_mf, E * 4);
  get(io->delays, x.delays, T * E * 4);
  get(io->truncated, x.truncated, E * 4);
  if (h->be.sync()) return fail(std::string("sfl_env_step: ") + h->be.error());
  return check_errors(h);
}

// sfl_env_step_dev: the same step with the caller's device buffers as the kernel's SflExt (a field the caller
// leaves null goes to the handle's own buffer) and the dense observation decoded behind it (env_encode_item),
// queued on the handle's stream without a wait; the envs' error flags stay in st.err for sfl_env_sync
template <class B>
int env_step_dev(Handle<B>* h, const sfl_env_dev_io* dio) {
  if (!h->env_mode) return fail("sfl_env_step_dev: call sfl_env_begin first");
  if (!dio) return fail("sfl_env_step_dev: null argument");
  if (h->max_na > SFL_MAX_ACTIONS)
    return fail("sfl_env_step_dev: the map has a switch with more than SFL_MAX_ACTIONS actions (the dense action mask "
                "cannot hold it)");
  if (((uintptr_t)dio->obs & 7u) || ((uintptr_t)dio->action_mask & 15u))
    return fail("sfl_env_step_dev: obs must be 8-byte and action_mask 16-byte aligned");
  if (h->E > 0xFFFFFFFFu / (uint32_t)OBS_PAIRS) return fail("sfl_env_step_dev: too many envs");
  const sfl_env_io& io = dio->io;
  const SflExt& own = h->ext;
  SflExt x{};
  // the actions go through the handle's own buffer (a stream-ordered device-to-device copy): a policy hands over a
  // fresh tensor every call, and the kernel's parameter block stays the previous call's (no upload, no wait)
  x.actions = own.actions;
  if (io.actions) h->be.d2d((void*)own.actions, io.actions, (size_t)h->E * 4);
  else h->be.memset((void*)own.actions, 0xFF, (size_t)h->E * 4);
  x.agent = io.agent ? io.agent : own.agent;
  x.train = io.train ? io.train : own.train;
  x.slot = io.slot ? io.slot : own.slot;
  x.state = io.state ? io.state : own.state;
  x.mask = io.mask ? io.mask : own.mask;
  x.reward = io.reward ? io.reward : own.reward;
  x.now = io.now ? io.now : own.now;
  x.next_sw = io.next_switch ? io.next_switch : own.next_sw;
  x.step_now = io.step_now ? io.step_now : own.step_now;
  x.arrived = io.arrived ? io.arrived : own.arrived;
  x.n_mf = io.malfunctions ? io.malfunctions : own.n_mf;
  x.delays = io.delays ? io.delays : own.delays;
  x.truncated = io.truncated ? io.truncated : own.truncated;
  SflEnc enc{};
  enc.E = h->E;
  enc.K = h->map.dec.K;
  enc.agent = x.agent;
  enc.slot = x.slot;
  enc.state = x.state;
  enc.mask = x.mask;
  enc.sw_np = h->map.sw_np;
  enc.sw_na = h->map.sw_na;
  enc.sw_rc = h->d_sw_rc;
  enc.st_rc = h->d_st_rc;
  enc.obs = dio->obs;
  enc.amask = dio->action_mask;
  enc.n_actions = dio->n_actions;
  enc.done = dio->done;
  SflCtl c{};
  c.mode = 2;
  c.launch_dec = h->d_launch_dec;
  c.launch_ticks = h->d_launch_ticks;
  c.launch_bytes = h->d_launch_bytes;
  if (h->be.run_ext_dev(h->map, h->st, c, x, enc, h->variant)) return fail(std::string("sfl_env_step_dev: ") + h->be.error());
  return trans_after_step(h, x);
}

// sfl_env_sync: wait for the handle's stream and report the envs' error flags as sfl_env_step does (the
// launch counters stay as the last host call left them)
template <class B>
int env_sync(Handle<B>* h) {
  if (!h->env_mode) return fail("sfl_env_sync: call sfl_env_begin first");
  uint64_t out[4] = {0, 0, 0, 0};
  h->be.reduce_launch(h->d_launch_dec, h->d_launch_ticks, h->d_launch_bytes, h->st.err, h->E, h->d_sums);
  h->be.d2h(out, h->d_sums, sizeof out);
  if (h->be.sync()) return fail(std::string("sfl_env_sync: ") + h->be.error());
  h->last_err = (uint32_t)out[3];
  return scan_errors(h);
}

template <class B>
int get_obs_tables(Handle<B>* h, int32_t* switch_rc, int32_t* station_rc) {
  if (switch_rc) h->be.d2h(switch_rc, h->d_sw_rc, (size_t)h->map.lrn.S * 8);
  if (station_rc) h->be.d2h(station_rc, h->d_st_rc, (size_t)h->map.dec.K * 8);
  return h->be.sync() ? fail(h->be.error()) : 0;
}

}  // namespace sfl

namespace sfl {

// ---------------------------------------------------------------------------
// graph-partitioned mode (sfl_part.h): owned Q storage and one round's three steps
// ---------------------------------------------------------------------------
template <class B>
int part_config(Handle<B>* h, int rank, int world, const int32_t* owner, uint32_t env_base, uint32_t E_tot,
                uint32_t cap_req, uint32_t cap_upd) {
  if (h->bank.on) return fail("sfl_part_config: an evaluation handle has no per-env table to partition (sfl_create_eval)");
  if (world < 1 || rank < 0 || rank >= world || world > 255) return fail("sfl_part_config: bad rank / world");
  if (h->part.world) return fail("sfl_part_config: already configured");
  if (h->map.env_group) return fail("sfl_part_config: the handle has hyperparameter groups (sfl_set_hparam_groups)");
  if (h->map.seed_sched) return fail("sfl_part_config: the handle has a seed schedule (sfl_set_seed_schedule)");
  if (env_base + h->E > E_tot) return fail("sfl_part_config: env range outside envs_total");
  if (cap_req < h->E) return fail("sfl_part_config: request capacity must hold one request per local env");
  if (cap_upd < 1 || (uint64_t)cap_req + cap_upd >= (1ull << 31) || (uint64_t)world * (cap_req + cap_upd + 1ull) >= (1ull << 32))
    return fail("sfl_part_config: bad capacities");
  // the wave kernel stages up to upd_env update records per env and round (E_MSG_OVF beyond); the
  // segments must hold every env's staged records
  const uint32_t upd_env = cap_upd / h->E < PART_UPD_ENV_MAX ? cap_upd / h->E : PART_UPD_ENV_MAX;
  if (upd_env < 2) return fail("sfl_part_config: update capacity must allow two records per local env");
  const int S = h->map.lrn.S, K = h->map.dec.K;
  std::vector<int32_t> own(owner, owner + S);
  for (int s = 0; s < S; ++s)
    if (own[s] < 0 || own[s] >= world) return fail("sfl_part_config: owner out of range");
  std::vector<uint64_t> qo(4 * (size_t)S, 0);
  std::vector<uint32_t> ro(4 * (size_t)S, 0);
  uint64_t off = 0;
  uint32_t rows = 0;
  for (int s = 0; s < S; ++s) {
    if (own[s] != rank) continue;
    const int P = h->h_sw_np[s];
    for (int i = 0; i < P; ++i) {
      const int g = 4 * s + i;
      const uint32_t nrows = (uint32_t)(1u << P) * (uint32_t)K * 3u;
      qo[g] = off;
      ro[g] = rows;
      off += (uint64_t)nrows * h->h_q_w[g];
      rows += nrows;
    }
  }
  // the env-local Q-table is not used in this mode: release it before the owned tables
  h->be.sync();
  h->dfree(h->st.lrn.q);
  h->dfree(h->st.lrn.touched);
  h->st.lrn.q = nullptr;
  h->st.lrn.touched = nullptr;
  SflPart& P = h->part;
  P.rank = rank;
  P.world = world;
  P.n_sw = S;
  P.env_base = env_base;
  P.E_tot = E_tot;
  // a segment holds one group per env of a source rank: its request and its update records to this
  // destination (cap_req >= the largest rank's env count, cap_upd its update records)
  P.cap_msg = cap_req + cap_upd;
  P.k_msg = P.cap_msg;  // (full segments until sfl_part_set_caps)
  P.q_own_per_env = off;
  P.own_rows = rows;
  P.own_words = (rows + 31u) / 32u;
  P.owner = h->upload(own.data(), own.size());
  std::vector<uint32_t> loc(S);
  for (int s = 0; s < S; ++s) loc[s] = own[s] == rank ? 1u : 0u;
  P.local_sw = h->upload(loc.data(), loc.size());
  P.q_off_own = h->upload(qo.data(), qo.size());
  P.row_own = h->upload(ro.data(), ro.size());
  P.q_own = h->template dalloc<double>((size_t)E_tot * (off ? off : 1));
  P.touched_own = h->template dalloc<uint32_t>((size_t)E_tot * (P.own_words ? P.own_words : 1));
  P.obs = h->template dalloc<Obs>(h->E);
  P.req_ix = h->template dalloc<uint32_t>(h->E);
  P.dec_done = h->template dalloc<int64_t>(h->E);
  P.cnt = h->template dalloc<uint32_t>((size_t)world + 4);
  P.sums = h->d_sums;
  P.cnt_out = h->template dalloc<uint64_t>(4 + ((size_t)PART_NCNT(world) + 1) / 2);
  P.upd_env = upd_env;
  P.req_st = h->template dalloc<PartReq>(h->E);
  P.req_dst = h->template dalloc<int32_t>(h->E);
  P.upd_st = h->template dalloc<PartUpd>((size_t)h->E * upd_env);
  P.upd_n = h->template dalloc<uint32_t>(h->E);
  P.eblk = nullptr;
  if (!P.owner || !P.q_own || !P.touched_own || !P.obs || !P.req_ix || !P.dec_done || !P.cnt || !P.cnt_out || !P.req_st ||
      !P.req_dst || !P.upd_st || !P.upd_n)
    return fail("sfl_part_config: allocation failed (out of memory?)");
  P.blocks_done = P.cnt + world;
  h->be.memset(P.cnt, 0, ((size_t)world + 4) * 4);
  h->be.memset(P.sums, 0, 4 * 8);
  h->be.memset(P.cnt_out, 0, (4 + ((size_t)PART_NCNT(world) + 1) / 2) * 8);
  h->be.fill_f64(P.q_own, h->map.dec.default_q, (size_t)E_tot * off);
  h->be.memset(P.touched_own, 0, (size_t)E_tot * P.own_words * 4);
  h->be.memset(P.dec_done, 0, h->E * 8);
  // a grouped shape (G < 64) becomes its one-env-per-wavefront shape: same env-major state layout
  if (h->variant > 0 && kVariants[h->variant].G != 64) h->variant = wave64_variant(h->map.lrn.S, h->map.T);
  if (h->variant > 0) {  // the wave kernels keep each env's scalars in a block between rounds
    P.eblk = h->template dalloc<uint32_t>((size_t)h->E * PART_EB);
    if (!P.eblk) return fail("sfl_part_config: allocation failed (out of memory?)");
  }
  h->eblk_state = 0;
  // the partitioned rounds run the body the handle was created for (h->variant: k_wave where
  // eligible, else the lane-per-env body), with that body's (switch, train) slot layout
  return h->be.sync() ? fail(h->be.error()) : 0;
}

// Q-init patch rows on the owned blocks (sfl_apply_qinit for a partitioned handle)
template <class B>
int part_qinit(Handle<B>* h, uint32_t n_rows, const uint32_t* row_port, const uint32_t* row_state, const double* values) {
  SflPart& P = h->part;
  const int rank = P.rank;
  std::vector<int32_t> own(h->map.lrn.S);
  h->be.d2h(own.data(), P.owner, own.size() * 4);
  if (h->be.sync()) return fail(h->be.error());
  // apply on the host copy of one env's owned table, then replicate over all envs
  std::vector<uint64_t> qo(4 * (size_t)h->map.lrn.S);
  std::vector<uint32_t> ro(4 * (size_t)h->map.lrn.S);
  h->be.d2h(qo.data(), P.q_off_own, qo.size() * 8);
  h->be.d2h(ro.data(), P.row_own, ro.size() * 4);
  if (h->be.sync()) return fail(h->be.error());
  std::vector<double> tab(P.q_own_per_env, h->map.dec.default_q);
  std::vector<uint32_t> bits(P.own_words, 0u);
  for (uint32_t r = 0; r < n_rows; ++r) {
    const uint32_t g = row_port[r], st = row_state[r];
    if (own[g >> 2] != rank) continue;
    const int w = h->h_q_w[g];
    for (int j = 0; j < w; ++j) {
      const double v = values[(size_t)r * 4 + j];
      tab[qo[g] + (size_t)st * w + j] = (v != v) ? h->map.dec.default_q : v;
    }
    const uint32_t rid = ro[g] + st;
    bits[rid >> 5] |= 1u << (rid & 31u);
  }
  // one env's owned table and key set, replicated over every env of the job
  if (P.q_own_per_env) {
    h->be.h2d(P.q_own, tab.data(), tab.size() * 8);
    h->be.replicate(P.q_own, tab.size() * 8, P.E_tot);
  }
  if (P.own_words) {
    h->be.h2d(P.touched_own, bits.data(), bits.size() * 4);
    h->be.replicate(P.touched_own, bits.size() * 4, P.E_tot);
  }
  return h->be.sync() ? fail(h->be.error()) : 0;
}

// one env of the job (global index): its owned Q blocks in the full per-env layout (other
// entries untouched) and its owned key-set bits OR-ed into `touched`
template <class B>
int part_get_q(Handle<B>* h, uint32_t genv, double* q, uint32_t* touched) {
  SflPart& P = h->part;
  if (genv >= P.E_tot) return fail("sfl_part_get_q: env out of range");
  std::vector<int32_t> own(h->map.lrn.S);
  std::vector<uint64_t> qo(4 * (size_t)h->map.lrn.S);
  std::vector<uint32_t> ro(4 * (size_t)h->map.lrn.S);
  std::vector<double> tab(P.q_own_per_env);
  std::vector<uint32_t> bits(P.own_words);
  h->be.d2h(own.data(), P.owner, own.size() * 4);
  h->be.d2h(qo.data(), P.q_off_own, qo.size() * 8);
  h->be.d2h(ro.data(), P.row_own, ro.size() * 4);
  if (P.q_own_per_env) h->be.d2h(tab.data(), P.q_own + (size_t)genv * P.q_own_per_env, tab.size() * 8);
  if (P.own_words) h->be.d2h(bits.data(), P.touched_own + (size_t)genv * P.own_words, bits.size() * 4);
  if (h->be.sync()) return fail(h->be.error());
  const int K = h->map.dec.K;
  for (int s = 0; s < h->map.lrn.S; ++s) {
    if (own[s] != P.rank) continue;
    const int np = h->h_sw_np[s];
    for (int i = 0; i < np; ++i) {
      const int g = 4 * s + i;
      const uint32_t nrows = (uint32_t)(1u << np) * (uint32_t)K * 3u;
      const int w = h->h_q_w[g];
      if (q) memcpy(q + h->h_q_off[g], tab.data() + qo[g], (size_t)nrows * w * 8);
      if (touched)
        for (uint32_t r = 0; r < nrows; ++r) {
          const uint32_t lr = ro[g] + r;
          if ((bits[lr >> 5] >> (lr & 31u)) & 1u) {
            const uint32_t fr = h->h_row_base[g] + r;
            touched[fr >> 5] |= 1u << (fr & 31u);
          }
        }
    }
  }
  return 0;
}

template <class B>
int part_begin(Handle<B>* h) {
  if (!h->part.world) return fail("sfl_part_begin: handle not partitioned");
  if (int rc = part_host_access(h, true)) return rc;
  h->be.memset(h->part.dec_done, 0, h->E * 8);
  return h->be.sync() ? fail(h->be.error()) : 0;
}

// this round's segment size (records per destination, without the header): the buffers handed to the
// next rounds hold [world][k + 1] records.  Every rank of the job must use the same value.
template <class B>
int part_set_caps(Handle<B>* h, uint32_t k_msg) {
  SflPart& P = h->part;
  if (!P.world) return fail("sfl_part_set_caps: handle not partitioned");
  if (k_msg < 1 || k_msg > P.cap_msg) return fail("sfl_part_set_caps: capacity outside [1, the configured capacity]");
  P.k_msg = k_msg;
  h->be.part_caps(P);
  return h->be.error()[0] ? fail(std::string("sfl_part_set_caps: ") + h->be.error()) : 0;
}

// the host copy of the last part_local's record counts, of the peaks and deferrals and of the launch
// totals accumulated since the previous read: a checkpoint's one synchronisation
template <class B>
int part_read(Handle<B>* h) {
  SflPart& P = h->part;
  std::vector<uint64_t> out(4 + ((size_t)PART_NCNT(P.world) + 1) / 2);
  h->be.d2h_async(out.data(), P.cnt_out, out.size() * 8);
  h->be.memset(P.cnt_out, 0, out.size() * 8);
  if (h->be.sync()) return fail(std::string("sfl_part_local: ") + h->be.error());
  h->part_pending = false;
  h->part_reads++;
  h->last_kernel_ms = h->be.elapsed_ms();
  h->last_dec = out[0];
  h->last_ticks = out[1];
  h->last_bytes = out[2];
  h->last_err = (uint32_t)out[3];
  h->total_dec += out[0];
  const uint32_t* cnt = (const uint32_t*)(out.data() + 4);
  const int W = P.world;
  std::vector<uint32_t> prev;
  if (!h->part_consumed) prev.swap(h->part_counts);  // (peaks and deferrals since sfl_part_counts: merged)
  h->part_counts.assign(cnt, cnt + PART_NCNT(W));
  if (prev.size() == h->part_counts.size()) {
    for (int i = PART_C_PEAK(W); i < PART_C_OPEN(W); ++i) h->part_counts[i] = std::max(h->part_counts[i], prev[i]);
    h->part_counts[PART_C_DEFER_SUM(W)] += prev[PART_C_DEFER_SUM(W)];
  }
  h->part_consumed = false;
  return scan_errors(h);
}

// local step of a round: every env applies its reply, runs to its next decision and emits the
// request (and the update records of its post step).  With n_req, one host synchronisation for
// the record counts and launch totals; without it on the caller's stream (sfl_set_stream), none:
// sfl_part_counts reads them later (errors of the envs surface there)
template <class B>
int part_local(Handle<B>* h, int64_t budget, const void* rep_in, void* msg_out, uint64_t* n_req) {
  SflPart& P = h->part;
  if (!P.world) return fail("sfl_part_local: handle not partitioned");
  P.rep_in = (const PartRep*)rep_in;
  P.msg_out = (PartMsg*)msg_out;
  SflCtl c{};
  c.mode = 0;
  c.ep_target = -1;
  c.dec_budget = budget;
  c.launch_dec = h->d_launch_dec;
  c.launch_ticks = h->d_launch_ticks;
  c.launch_bytes = h->d_launch_bytes;
  float ms = 0.f;
  if (P.eblk && h->eblk_state == 0) h->be.part_eblk(h->st, P, 0);  // (stream-ordered before the launch)
  if (h->be.part_local(h->map, h->st, c, P, h->variant, &ms)) return fail(std::string("sfl_part_local: ") + h->be.error());
  if (P.eblk) h->eblk_state = 1;
  h->part_pending = true;
  if (!n_req) return 0;  // (sfl_part_counts reads them)
  if (int rc = part_read(h)) return rc;
  if (n_req) *n_req = h->part_counts[PART_C_OPEN(P.world)];
  return 0;
}

// the owner steps are queued without a synchronisation when the caller's stream carries the
// round (sfl_set_stream): launch errors still surface, kernel faults at the next synchronisation
template <class B>
int part_done(Handle<B>* h, const char* what) {
  if (h->ext_stream) return h->be.error()[0] ? fail(std::string(what) + ": " + h->be.error()) : 0;
  return h->be.sync() ? fail(std::string(what) + ": " + h->be.error()) : 0;
}

// the owner side of a round on the received segments: each env's update records in order, then the
// answer to its request (sfl_part.h part_owner_group)
template <class B>
int part_owner(Handle<B>* h, const void* msg_in, void* rep_out) {
  SflPart& P = h->part;
  if (!P.world) return fail("sfl_part_owner: handle not partitioned");
  h->be.part_owner(h->map, P, (const PartMsg*)msg_in, (PartRep*)rep_out);
  return part_done(h, "sfl_part_owner");
}

// which switches' rows the wave kernel decides on and updates directly: local[S] (null: the
// switches this rank owns, the default), the rest through their owners' messages.  Rows of
// another rank's switch cannot be local; marking fewer of this rank's own switches local
// rehearses a bigger job's message traffic on one rank.  The lane-per-env body always sends.
template <class B>
int part_set_local_rows(Handle<B>* h, const uint8_t* local) {
  SflPart& P = h->part;
  if (!P.world) return fail("sfl_part_set_local_rows: handle not partitioned");
  const int S = h->map.lrn.S;
  std::vector<int32_t> own(S);
  h->be.d2h(own.data(), P.owner, own.size() * 4);
  if (h->be.sync()) return fail(h->be.error());
  std::vector<uint32_t> loc(S);
  for (int s = 0; s < S; ++s) {
    const bool want = local ? local[s] != 0 : own[s] == P.rank;
    if (want && own[s] != P.rank) return fail("sfl_part_set_local_rows: switch owned by another rank marked local");
    loc[s] = want ? 1u : 0u;
  }
  h->be.h2d((void*)P.local_sw, loc.data(), loc.size() * 4);
  return h->be.sync() ? fail(h->be.error()) : 0;
}

// this rank's counts (sfl_part.h PART_C_*): of the last part_local, message records staged per destination,
// then their peaks per destination since the previous read, that round's open and deferred envs and the
// deferrals since the previous read.  cap >= world (the first counts only)
template <class B>
int part_counts(Handle<B>* h, uint32_t* out, int32_t cap) {
  if (!h->part.world) return fail("sfl_part_counts: handle not partitioned");
  const int32_t n = PART_NCNT(h->part.world);
  if (cap < h->part.world) return fail("sfl_part_counts: buffer too small");
  if (h->part_pending)
    if (int rc = part_read(h)) return rc;
  for (int32_t i = 0; i < n && i < cap; ++i) out[i] = i < (int32_t)h->part_counts.size() ? h->part_counts[i] : 0u;
  h->part_consumed = true;
  return 0;
}

// ---------------------------------------------------------------------------
// consensus Q-tables (include/sfl.h sfl_consensus; sfl_consensus.h; DESIGN.md "Consensus Q-tables")
// ---------------------------------------------------------------------------
// Partial records (sum, first pattern, meta: 20 bytes a cell) exist only for the chunks of cohorts of more than
// SFL_CONSENSUS_CHUNK members, at most 2 E / SFL_CONSENSUS_CHUNK chunks: the scratch is at most
// 2 E / 256 * q_per_env * 20 bytes, 2 % of the Q block, allocated for the call and freed.
template <class B>
int consensus(Handle<B>* h, int32_t mode, uint32_t flags, uint32_t n_cohorts, const uint32_t* env_cohort, double* kernel_ms) {
  if (mode != SFL_CONSENSUS_MEAN && mode != SFL_CONSENSUS_MAX)
    return fail("sfl_consensus: mode " + std::to_string(mode) + " (SFL_CONSENSUS_MEAN or SFL_CONSENSUS_MAX)");
  if (h->bank.on) return fail("sfl_consensus: an evaluation handle has no per-env tables to merge (sfl_create_eval)");
  if (flags & ~(uint32_t)SFL_CONSENSUS_SHARE) return fail("sfl_consensus: unknown flag bits");
  if (h->part.world) return fail("sfl_consensus: the handle is graph-partitioned (its tables are owned rows)");
  if (h->env_mode) return fail("sfl_consensus: the handle is in external-action mode (no learner)");
  const uint32_t E = h->E;
  if (n_cohorts == 0 || n_cohorts > E)
    return fail("sfl_consensus: n_cohorts " + std::to_string(n_cohorts) + " outside [1, n_envs = " + std::to_string(E) + "]");
  if (env_cohort)
    for (uint32_t e = 0; e < E; ++e)
      if (env_cohort[e] >= n_cohorts && env_cohort[e] != SFL_NO_COHORT)
        return fail("sfl_consensus: env " + std::to_string(e) + " is in cohort " + std::to_string(env_cohort[e]) + " of " +
                    std::to_string(n_cohorts));
  const SflMap& m = h->map;
  const uint64_t Q = m.lrn.q_per_env;
  const uint32_t tw = m.lrn.touched_words;
  if (!h->d_cell_row) {
    // each cell's row id, as k_qinit derives it: block g holds rows row_base[g] + state, q_w[g] cells each
    std::vector<uint32_t> cr(Q ? Q : 1, CONS_NO_ROW);
    for (int s = 0; s < m.lrn.S; ++s)
      for (int i = 0; i < (int)h->h_sw_np[s]; ++i) {
        const size_t g = (size_t)s * 4 + i;
        const uint64_t w = h->h_q_w[g], nrows = ((uint64_t)1 << h->h_sw_np[s]) * (uint64_t)m.dec.K * 3u;
        if (w == 0) continue;
        if (h->h_q_off[g] + nrows * w > Q || h->h_row_base[g] + nrows > m.rows_per_env)
          return fail("sfl_consensus: a Q block lies outside the env's table (map compiler mismatch)");
        for (uint64_t r = 0; r < nrows; ++r)
          for (uint64_t j = 0; j < w; ++j) cr[h->h_q_off[g] + r * w + j] = h->h_row_base[g] + (uint32_t)r;
      }
    uint32_t* d = (uint32_t*)h->upload(cr.data(), cr.size());
    if (!d || h->be.sync()) {
      if (d) h->dfree(d);
      return fail("sfl_consensus: device allocation failed (cell rows)");
    }
    h->d_cell_row = d;
  }
  if (h->cons_n != n_cohorts) {
    if (h->cons_q) h->dfree(h->cons_q);
    if (h->cons_keys) h->dfree(h->cons_keys);
    h->cons_n = 0;
    h->cons_q = h->template dalloc<double>((size_t)n_cohorts * Q);
    h->cons_keys = h->template dalloc<uint32_t>((size_t)n_cohorts * tw);
    if (!h->cons_q || !h->cons_keys) {
      if (h->cons_q) h->dfree(h->cons_q);
      if (h->cons_keys) h->dfree(h->cons_keys);
      h->cons_q = nullptr;
      h->cons_keys = nullptr;
      return fail("sfl_consensus: device allocation failed (consensus tables)");
    }
  }
  // member lists: the envs of each cohort in ascending order, cohort after cohort; their chunks as jobs
  std::vector<uint32_t> off(n_cohorts + 1, 0u), members;
  for (uint32_t e = 0; e < E; ++e) {
    const uint32_t c = env_cohort ? env_cohort[e] : 0u;
    if (c != SFL_NO_COHORT) ++off[c + 1];
  }
  for (uint32_t c = 0; c < n_cohorts; ++c) off[c + 1] += off[c];
  members.resize(off[n_cohorts] ? off[n_cohorts] : 1);
  {
    std::vector<uint32_t> at(off.begin(), off.end() - 1);
    for (uint32_t e = 0; e < E; ++e) {
      const uint32_t c = env_cohort ? env_cohort[e] : 0u;
      if (c != SFL_NO_COHORT) members[at[c]++] = e;
    }
  }
  std::vector<ConsJob> jobs;
  std::vector<ConsCombo> combos;
  uint32_t n_slots = 0;
  for (uint32_t c = 0; c < n_cohorts; ++c) {
    const uint32_t n = off[c + 1] - off[c];
    if (n <= SFL_CONSENSUS_CHUNK) {
      jobs.push_back(ConsJob{off[c], n, c, CONS_DIRECT});
      continue;
    }
    const uint32_t chunks = (n + SFL_CONSENSUS_CHUNK - 1) / SFL_CONSENSUS_CHUNK;
    combos.push_back(ConsCombo{n_slots, chunks, c, 0u});
    for (uint32_t k = 0; k < chunks; ++k) {
      const uint32_t b = k * SFL_CONSENSUS_CHUNK;
      jobs.push_back(ConsJob{off[c] + b, std::min<uint32_t>(SFL_CONSENSUS_CHUNK, n - b), c, n_slots++});
    }
  }
  ConsArgs a{};
  a.mode = mode;
  a.flags = flags;
  a.E = E;
  a.n_cohorts = n_cohorts;
  a.tw = tw;
  a.n_jobs = (uint32_t)jobs.size();
  a.n_combos = (uint32_t)combos.size();
  a.n_slots = n_slots;
  a.Q = Q;
  a.default_bits = cons_bits(m.dec.default_q);
  const uint64_t q_tiles = (Q + CONS_TILE - 1) / CONS_TILE;
  a.cells_cap = q_tiles * CONS_TILE;
  a.q = h->st.lrn.q;
  a.touched = h->st.lrn.touched;
  a.cell_row = h->d_cell_row;
  a.cons_q = h->cons_q;
  a.cons_keys = h->cons_keys;
  std::vector<void*> scratch;
  auto up = [&](const void* src, size_t bytes) -> void* {
    void* p = h->be.alloc(bytes ? bytes : 1);
    scratch.push_back(p);
    if (p && bytes && src) h->be.h2d(p, src, bytes);
    return p;
  };
  a.members = (const uint32_t*)up(members.data(), members.size() * 4);
  a.coh_off = (const uint32_t*)up(off.data(), off.size() * 4);
  a.jobs = (const ConsJob*)up(jobs.data(), jobs.size() * sizeof(ConsJob));
  a.combos = (const ConsCombo*)up(combos.data(), combos.size() * sizeof(ConsCombo));
  if (n_slots && B::kConsPartials) {
    const size_t recs = (size_t)n_slots * a.cells_cap;
    a.p_sum = (double*)up(nullptr, recs * 8);
    a.p_first = (uint64_t*)up(nullptr, recs * 8);
    a.p_meta = (uint32_t*)up(nullptr, recs * 4);
    a.p_keys = (uint32_t*)up(nullptr, (size_t)n_slots * tw * 4);
  }
  bool ok = true;
  for (void* p : scratch) ok = ok && p;
  float ms = 0.f;
  int rc = ok ? h->be.consensus(a, &ms) : -1;
  if (h->be.sync()) rc = -1;  // (the host sources of the uploads live until here)
  for (void* p : scratch) h->be.free(p);
  if (!ok) return fail("sfl_consensus: device allocation failed (member lists or partial records)");
  if (rc) return fail(std::string("sfl_consensus: ") + h->be.error());
  h->cons_n = n_cohorts;
  if (kernel_ms) *kernel_ms = ms;
  return 0;
}

template <class B>
int get_consensus_q(Handle<B>* h, uint32_t cohort, double* q, uint32_t* touched) {
  if (h->part.world) return fail("sfl_get_consensus_q: the handle is graph-partitioned");
  if (h->env_mode) return fail("sfl_get_consensus_q: the handle is in external-action mode (no learner)");
  if (!h->cons_n) return fail("sfl_get_consensus_q: no sfl_consensus call yet");
  if (cohort >= h->cons_n)
    return fail("sfl_get_consensus_q: cohort " + std::to_string(cohort) + " of " + std::to_string(h->cons_n));
  const size_t Q = h->map.lrn.q_per_env, tw = h->map.lrn.touched_words;
  if (q) h->be.d2h(q, h->cons_q + (size_t)cohort * Q, Q * 8);
  if (touched) h->be.d2h(touched, h->cons_keys + (size_t)cohort * tw, tw * 4);
  return h->be.sync() ? fail(h->be.error()) : 0;
}

// ---------------------------------------------------------------------------
// step-mode learning curves (include/sfl.h sfl_curve_*; sfl_curve.h)
// ---------------------------------------------------------------------------
template <class B>
int curve_end(Handle<B>* h) {
  if (!h->cv.on) return fail("sfl_curve_end: the handle has no curve (sfl_curve_begin)");
  if (h->be.sync()) return fail(h->be.error());
  const CurveArgs& a = h->cv.a;
  const CurveXArgs& x = h->cv.xa;  // (all null without an exploit record)
  for (const void* p : {(const void*)x.mark, (const void*)x.sx_cum, (const void*)x.sx_arrived, (const void*)x.cells,
                        (const void*)h->cv.x_limit})
    if (p) h->dfree((void*)p);
  for (const void* p : {(const void*)a.mark, (const void*)a.series, (const void*)a.st_cum, (const void*)a.st_arrived,
                        (const void*)a.st_mf, (const void*)a.st_dec, (const void*)a.st_ticks, (const void*)a.st_delays,
                        (const void*)a.cells})
    if (p) h->dfree((void*)p);
  h->cv = typename Handle<B>::Curve{};
  return 0;
}

template <class B>
int curve_begin(Handle<B>* h, int32_t bin_episodes, int32_t n_bins, uint32_t n_series, const uint32_t* env_series,
                int32_t ring_cap) {
  if (h->bank.on) return fail("sfl_curve_begin: an evaluation handle has no sfl_step to fold (sfl_create_eval)");
  if (h->part.world) return fail("sfl_curve_begin: the handle is graph-partitioned (sfl_part_local records no episodes)");
  if (h->env_mode) return fail("sfl_curve_begin: the handle is in external-action mode (sfl_env_begin): no sfl_step to fold");
  if (bin_episodes < 1 || n_bins < 1 || n_series < 1 || ring_cap < 1)
    return fail("sfl_curve_begin: bin_episodes, n_bins, n_series and ring_cap must be at least 1");
  const size_t E = h->E, T = (size_t)h->map.T;
  const uint64_t table_bytes = (uint64_t)n_bins * n_series * sizeof(sfl_curve_cell);
  if (table_bytes > SFL_CURVE_MAX_TABLE_BYTES)
    return fail("sfl_curve_begin: n_bins * n_series cells take " + std::to_string(table_bytes) + " bytes, above " +
                std::to_string(SFL_CURVE_MAX_TABLE_BYTES) + " (SFL_CURVE_MAX_TABLE_BYTES)");
  const uint64_t ring_bytes = (uint64_t)ring_cap * E * (24 + 4 * T);
  if (ring_bytes > SFL_CURVE_MAX_RING_BYTES)
    return fail("sfl_curve_begin: a ring of " + std::to_string(ring_cap) + " rows takes " + std::to_string(ring_bytes) +
                " bytes, above " + std::to_string(SFL_CURVE_MAX_RING_BYTES) + " (SFL_CURVE_MAX_RING_BYTES)");
  std::vector<uint32_t> ser(E, 0u);
  if (env_series) {
    for (size_t e = 0; e < E; ++e) {
      if (env_series[e] >= n_series)
        return fail("sfl_curve_begin: env " + std::to_string(e) + " is in series " + std::to_string(env_series[e]) + " of " +
                    std::to_string(n_series));
      ser[e] = env_series[e];
    }
  } else if (h->map.env_group) {
    if (n_series != (uint32_t)h->map.n_groups)
      return fail("sfl_curve_begin: n_series " + std::to_string(n_series) + " is not the handle's group count " +
                  std::to_string(h->map.n_groups) + " (env_series == NULL takes each env's hyperparameter group)");
    std::vector<uint16_t> eg(E);
    h->be.d2h(eg.data(), h->map.env_group, E * 2);
    if (h->be.sync()) return fail(h->be.error());
    for (size_t e = 0; e < E; ++e) ser[e] = eg[e];
  }
  if (h->cv.on)
    if (int rc = curve_end(h)) return rc;
  CurveArgs a{};
  a.E = h->E;
  a.n_series = n_series;
  a.T = h->map.T;
  a.n_bins = n_bins;
  a.bin_episodes = bin_episodes;
  a.ring_cap = ring_cap;
  a.max_steps = h->map.max_steps;
  a.ep_t = h->st.ep_t;
  const size_t R = (size_t)ring_cap;
  a.mark = h->template dalloc<int32_t>(E);
  a.series = h->template dalloc<uint32_t>(E);
  a.st_cum = h->template dalloc<double>(R * E);
  a.st_arrived = h->template dalloc<int32_t>(R * E);
  a.st_mf = h->template dalloc<int32_t>(R * E);
  a.st_dec = h->template dalloc<int32_t>(R * E);
  a.st_ticks = h->template dalloc<int32_t>(R * E);
  a.st_delays = h->template dalloc<int32_t>(R * T * E);
  a.cells = h->template dalloc<int64_t>((size_t)n_bins * n_series * CV_WORDS);
  h->cv.a = a;
  h->cv.on = true;  // (curve_end releases whatever was allocated)
  if (!a.mark || !a.series || !a.st_cum || !a.st_arrived || !a.st_mf || !a.st_dec || !a.st_ticks || !a.st_delays || !a.cells) {
    curve_end(h);
    return fail("sfl_curve_begin: device allocation failed (ring or cells)");
  }
  h->be.h2d((void*)a.series, ser.data(), E * 4);
  h->be.d2d(a.mark, h->st.ep_t, E * 4);  // the episodes before the curve are neither folded nor lost
  h->be.memset((void*)a.st_cum, 0, R * E * 8);
  h->be.memset((void*)a.st_arrived, 0, R * E * 4);
  h->be.memset((void*)a.st_mf, 0, R * E * 4);
  h->be.memset((void*)a.st_dec, 0, R * E * 4);
  h->be.memset((void*)a.st_ticks, 0, R * E * 4);
  h->be.memset((void*)a.st_delays, 0, R * T * E * 4);
  int rc = h->be.curve(a, true);
  if (h->be.sync()) rc = -1;  // (the host source of the series upload lives until here)
  if (rc) {
    curve_end(h);
    return fail(std::string("sfl_curve_begin: ") + h->be.error());
  }
  return 0;
}

template <class B>
int curve_read(Handle<B>* h, sfl_curve_cell* out) {
  if (!h->cv.on) return fail("sfl_curve_read: the handle has no curve (sfl_curve_begin)");
  if (!out) return fail("sfl_curve_read: null argument");
  const CurveArgs& a = h->cv.a;
  h->be.d2h(out, a.cells, (size_t)a.n_bins * a.n_series * sizeof(sfl_curve_cell));
  return h->be.sync() ? fail(h->be.error()) : 0;
}

template <class B>
int curve_episodes(Handle<B>* h, int32_t* out) {
  if (!h->cv.on) return fail("sfl_curve_episodes: the handle has no curve (sfl_curve_begin)");
  if (!out) return fail("sfl_curve_episodes: null argument");
  h->be.d2h(out, h->cv.a.mark, (size_t)h->E * 4);
  return h->be.sync() ? fail(h->be.error()) : 0;
}

// after sfl_learn: its episodes went to its own buffers; a later sfl_step folds only its own
template <class B>
int curve_skip_to_now(Handle<B>* h) {
  if (!h->cv.on) return 0;
  h->be.d2d(h->cv.a.mark, h->st.ep_t, (size_t)h->E * 4);
  if (h->be.sync()) return fail(h->be.error());
  return curve_exploit_sync(h);
}

// ---- the exploit record (include/sfl.h sfl_curve_exploit; sfl_curve.h) ----
static_assert(CVX_DONE == F_EXPLOIT_DONE, "sfl_curve.h reads F_EXPLOIT_DONE from the flags word");

// The marks set to the rounds every env has completed by now, so that the next fold takes up from here (a new record,
// after sfl_learn_begin, sfl_learn and sfl_mark_exploit_done).  After sfl_curve_exploit(h, 0) also the limits: an env
// completes the round it is in (its greedy flag holds until its next reset) and no other.
template <class B>
int curve_exploit_sync(Handle<B>* h) {
  if (!h->cv.x_on) return 0;
  const size_t E = h->E;
  CurveXArgs& x = h->cv.xa;
  std::vector<int32_t> ep(E), ph(E), mark(E), limit;
  std::vector<uint32_t> fl(E);
  h->be.d2h(ep.data(), h->st.ep_t, E * 4);
  h->be.d2h(ph.data(), h->st.phase, E * 4);
  h->be.d2h(fl.data(), h->st.eflags, E * 4);
  if (h->be.sync()) return fail(h->be.error());
  for (size_t e = 0; e < E; ++e) mark[e] = curve_rounds_done(ep[e], fl[e], x.f);
  h->be.h2d(x.mark, mark.data(), E * 4);
  x.limit = nullptr;
  if (h->cv.x_freq == 0) {
    limit.resize(E);
    for (size_t e = 0; e < E; ++e) {
      const bool in_flight = (fl[e] & F_GREEDY) && !(fl[e] & F_EXPLOIT_DONE) && ph[e] != PH_RESET;
      limit[e] = mark[e] + (in_flight ? 1 : 0);
    }
    h->be.h2d(h->cv.x_limit, limit.data(), E * 4);
    x.limit = h->cv.x_limit;
  }
  return h->be.sync() ? fail(h->be.error()) : 0;  // (the host sources of the uploads live until here)
}

template <class B>
int curve_exploit(Handle<B>* h, int32_t f) {
  if (f < 0) return fail("sfl_curve_exploit: exploit_freq must not be negative");
  if (!h->cv.on) return fail("sfl_curve_exploit: the handle has no curve (sfl_curve_begin)");
  if (f == 0) {  // no new round starts; the record stays
    if (!h->cv.x_on) return 0;
    h->cv.x_freq = 0;
    return curve_exploit_sync(h);
  }
  const CurveArgs& a = h->cv.a;
  const size_t E = h->E, R = (size_t)a.ring_cap;
  if (!h->cv.x_on) {
    const uint64_t ring_bytes = (uint64_t)a.ring_cap * E * (24 + 4 * (uint64_t)a.T + 12);
    if (ring_bytes > SFL_CURVE_MAX_RING_BYTES)
      return fail("sfl_curve_exploit: with the rounds' rows the ring of " + std::to_string(a.ring_cap) + " rows takes " +
                  std::to_string(ring_bytes) + " bytes, above " + std::to_string(SFL_CURVE_MAX_RING_BYTES) +
                  " (SFL_CURVE_MAX_RING_BYTES)");
    CurveXArgs x{};
    x.E = a.E;
    x.n_series = a.n_series;
    x.T = a.T;
    x.n_bins = a.n_bins;
    x.bin_episodes = a.bin_episodes;
    x.ring_cap = a.ring_cap;
    x.ep_t = h->st.ep_t;
    x.eflags = h->st.eflags;
    x.series = a.series;
    x.mark = h->template dalloc<int32_t>(E);
    x.sx_cum = h->template dalloc<double>(R * E);
    x.sx_arrived = h->template dalloc<int32_t>(R * E);
    x.cells = h->template dalloc<int64_t>((size_t)a.n_bins * a.n_series * XV_WORDS);
    h->cv.x_limit = h->template dalloc<int32_t>(E);
    h->cv.xa = x;
    if (!x.mark || !x.sx_cum || !x.sx_arrived || !x.cells || !h->cv.x_limit) {
      for (const void* p : {(const void*)x.mark, (const void*)x.sx_cum, (const void*)x.sx_arrived, (const void*)x.cells,
                            (const void*)h->cv.x_limit})
        if (p) h->dfree((void*)p);
      h->cv.xa = CurveXArgs{};
      h->cv.x_limit = nullptr;
      return fail("sfl_curve_exploit: device allocation failed (ring or cells)");
    }
    h->be.memset((void*)x.sx_cum, 0, R * E * 8);
    h->be.memset((void*)x.sx_arrived, 0, R * E * 4);
    h->cv.x_on = true;
  }
  CurveXArgs& x = h->cv.xa;
  int32_t g = a.ring_cap, r = f;  // gcd(ring_cap, f)
  while (r) {
    const int32_t t = g % r;
    g = r;
    r = t;
  }
  x.f = f;
  x.period = a.ring_cap / g;
  h->cv.x_freq = f;
  if (h->be.curve_exploit(x, true)) return fail(std::string("sfl_curve_exploit: ") + h->be.error());
  return curve_exploit_sync(h);
}

template <class B>
int curve_read_exploit(Handle<B>* h, sfl_curve_xcell* out) {
  if (!h->cv.x_on) return fail("sfl_curve_read_exploit: the handle has no exploit record (sfl_curve_exploit)");
  if (!out) return fail("sfl_curve_read_exploit: null argument");
  const CurveXArgs& x = h->cv.xa;
  h->be.d2h(out, x.cells, (size_t)x.n_bins * x.n_series * sizeof(sfl_curve_xcell));
  return h->be.sync() ? fail(h->be.error()) : 0;
}

template <class B>
int curve_rounds(Handle<B>* h, int32_t* out) {
  if (!h->cv.x_on) return fail("sfl_curve_rounds: the handle has no exploit record (sfl_curve_exploit)");
  if (!out) return fail("sfl_curve_rounds: null argument");
  h->be.d2h(out, h->cv.xa.mark, (size_t)h->E * 4);
  return h->be.sync() ? fail(h->be.error()) : 0;
}

// ---------------------------------------------------------------------------
// suspend and resume (include/sfl.h sfl_state_*; sfl_snap.h)
// ---------------------------------------------------------------------------
// The env's record: every SflState array except q / touched, in declaration order, each at an offset aligned to its
// element size; the layout class decides which arrays are env-major (sfl_wave.h tix / pix / cix, slot_ix) and that the
// semaphore records are the wave kernels' 32-bit ones.  Returns the record's bytes (a multiple of 8).
template <class B>
uint32_t snap_fields(Handle<B>* h, SnapField* f, uint32_t* n_fields, uint32_t* seed_off) {
  const SflState& s = h->st;
  const SflMap& m = h->map;
  const uint32_t T = (uint32_t)m.T, S = (uint32_t)m.lrn.S, NP = (uint32_t)m.NP, HW = (uint32_t)m.HW;
  const uint32_t wave = h->variant > 0 ? 1u : 0u;
  uint32_t n = 0, off = 0;
  auto add = [&](void* base, uint32_t elem, uint32_t count, uint32_t major) {
    off = (off + elem - 1u) / elem * elem;
    f[n++] = SnapField{base, elem, count, major, off};
    off += elem * count;
  };
  add(s.phase, 4, 1, 0);
  add(s.elapsed, 4, 1, 0);
  add(s.eflags, 4, 1, 0);
  add(s.ep_t, 4, 1, 0);
  add(s.n_test, 4, 1, 0);
  add(s.epoch, 4, 1, 0);
  add(s.rng, 8, 5, 0);
  *seed_off = (off + 7u) / 8u * 8u;
  add(s.seed, 8, 1, 0);
  add(s.cum_reward, 8, 1, 0);
  add(s.n_mf, 4, 1, 0);
  add(s.ep_dec, 4, 1, 0);
  add(s.ep_ticks, 4, 1, 0);
  add(s.step_ctr, 8, 1, 0);
  add(s.dec_total, 8, 1, 0);
  add(s.masks, 4, 4 * MAXW, 0);
  add(s.err, 4, 1, 0);
  add(s.tr_pos, 4, T, wave);
  add(s.tr_bits, 4, T, wave);
  add(s.tr_plan, 4, T, wave);
  add(s.tr_next, 2, T, wave);
  add(s.tr_prev, 2, T, wave);
  add(s.tr_src, 2, T, wave);
  add(s.tr_dec, 2, T, wave);
  add(s.tr_delay, 4, T, wave);
  // (the lane body's ownership lists, tick scratch and cell maps: the wave kernels never touch them)
  add(s.own, 2, T * OWN_MAX, 0);
  add(s.own_n, 1, T, 0);
  add(s.sc_desired, 4, T, 0);
  add(s.sc_pred, 4, T, 0);
  add(s.sc_aux, 4, T, 0);
  add(s.occ, 1, HW, 0);
  add(s.claim, 1, HW, 0);
  if (wave) add(s.sem, 4, NP, 1);  // (32-bit records [E][NP] in the array sized for the 64-bit ones)
  else add(s.sem, 8, NP, 0);
  add(s.lrn.slot, 8, S * T, wave);
  add(s.lrn.counts, 4, S, wave);
  // a handle with a seed schedule: the running episode's seed too (a call takes effect at the next reset only, so the
  // value does not follow from the schedule and the episode index).  Other handles' records are what they were.
  if (m.seed_sched) add(s.ep_seed, 8, 1, 0);
  static_assert(SNAP_MAX_FIELDS >= 36, "fields");
  *n_fields = n;
  return (off + 7u) / 8u * 8u;
}

template <class B>
uint64_t snap_fingerprint(Handle<B>* h) {
  const SflMap& m = h->map;
  uint64_t fp = snap_hash(0xCBF29CE484222325ull, &h->snap.map_fp, 8);
  fp = snap_hash(fp, &m.upd.gamma, 8);
  fp = snap_hash(fp, &m.dec.default_q, 8);
  const int64_t sc[] = {m.lrn.ntab, m.max_steps, m.dec.delay_thr, m.mf_steps > 0 ? 1 : 0, h->variant > 0 ? 1 : 0};
  fp = snap_hash(fp, sc, sizeof sc);
  if (m.seed_sched) {  // (its records carry one more field; an unscheduled handle's fingerprint is what it was)
    const int64_t sched = 1;
    fp = snap_hash(fp, &sched, sizeof sched);
  }
  return fp;
}

template <class B>
int snap_refuse(Handle<B>* h, const std::string& fn) {
  if (h->bank.on) return fail(fn + ": an evaluation handle has no per-env table (sfl_create_eval)");
  if (h->part.world) return fail(fn + ": the handle is graph-partitioned (its tables are owned rows)");
  if (h->env_mode) return fail(fn + ": the handle is in external-action mode (no learner)");
  if (h->map.lrn.q_per_env >= (1ull << 32)) return fail(fn + ": Q-table beyond 2^32 cells per env");
  return 0;
}

// each row's first cell and width, as k_qinit derives them: block g holds rows row_base[g] + state, q_w[g] cells each
template <class B>
int snap_tables(Handle<B>* h, const std::string& fn) {
  typename Handle<B>::Snap& sn = h->snap;
  if (sn.d_row_w) return 0;
  const SflMap& m = h->map;
  const uint32_t rows = m.rows_per_env;
  sn.row_w.assign(rows ? rows : 1, 0);
  sn.row_cell.assign(rows ? rows : 1, 0);
  for (int s = 0; s < m.lrn.S; ++s)
    for (int i = 0; i < (int)h->h_sw_np[s]; ++i) {
      const size_t g = (size_t)s * 4 + i;
      const uint64_t w = h->h_q_w[g], nrows = ((uint64_t)1 << h->h_sw_np[s]) * (uint64_t)m.dec.K * 3u;
      if (w == 0) continue;
      if (w > 4 || h->h_q_off[g] + nrows * w > m.lrn.q_per_env || h->h_row_base[g] + nrows > rows)
        return fail(fn + ": a Q block lies outside the env's table (map compiler mismatch)");
      for (uint64_t r = 0; r < nrows; ++r) {
        sn.row_w[h->h_row_base[g] + r] = (uint8_t)w;
        sn.row_cell[h->h_row_base[g] + r] = h->h_q_off[g] + r * w;
      }
    }
  uint8_t* dw = (uint8_t*)h->upload(sn.row_w.data(), sn.row_w.size());
  uint64_t* dc = (uint64_t*)h->upload(sn.row_cell.data(), sn.row_cell.size());
  if (!dw || !dc || h->be.sync()) {
    if (dw) h->dfree(dw);
    if (dc) h->dfree(dc);
    return fail(fn + ": device allocation failed (row table)");
  }
  sn.d_row_w = dw;
  sn.d_row_cell = dc;
  return 0;
}

template <class B>
void snap_drop(Handle<B>* h) {
  for (void* p : h->snap.bufs) h->be.free(p);
  h->snap.bufs.clear();
  h->snap.pending = false;
}

template <class B>
void snap_args(Handle<B>* h, SnapArgs& a, uint32_t n) {
  const SflMap& m = h->map;
  a = SnapArgs{};
  a.E = h->E;
  a.n = n;
  a.tw = m.lrn.touched_words;
  a.rows = m.rows_per_env;
  a.groups = (m.rows_per_env + SNAP_GROUP - 1) / SNAP_GROUP;
  uint32_t seed_off = 0;
  a.state_bytes = snap_fields(h, a.fields, &a.n_fields, &seed_off);
  a.Q = m.lrn.q_per_env;
  a.default_bits = cons_bits(m.dec.default_q);
  a.q = (uint64_t*)h->st.lrn.q;
  a.touched = h->st.lrn.touched;
  a.row_cell = h->snap.d_row_cell;
  a.row_w = h->snap.d_row_w;
}

template <class B>
int state_info(Handle<B>* h, sfl_state_desc* out) {
  if (!out) return fail("sfl_state_info: null argument");
  if (int rc = snap_refuse(h, "sfl_state_info")) return rc;
  SnapField f[SNAP_MAX_FIELDS];
  uint32_t nf = 0, seed_off = 0;
  memset(out, 0, sizeof *out);
  out->state_bytes = snap_fields(h, f, &nf, &seed_off);
  out->seed_offset = seed_off;
  out->fingerprint = snap_fingerprint(h);
  out->q_per_env = h->map.lrn.q_per_env;
  out->layout = h->variant > 0 ? SFL_STATE_WAVE : SFL_STATE_LANE;
  out->touched_words = h->map.lrn.touched_words;
  out->rows_per_env = h->map.rows_per_env;
  return 0;
}

// a list of envs / slots: in range, none twice
template <class B>
int snap_list(Handle<B>* h, const std::string& fn, const char* what, uint32_t n, const uint32_t* list) {
  if (n && !list) return fail(fn + ": null " + what + " list");
  if (n > h->E) return fail(fn + ": " + std::to_string(n) + " " + what + "s listed, the handle has " + std::to_string(h->E));
  std::vector<uint8_t> seen(h->E, 0);
  for (uint32_t k = 0; k < n; ++k) {
    if (list[k] >= h->E)
      return fail(fn + ": " + what + " " + std::to_string(list[k]) + " out of range (n_envs = " + std::to_string(h->E) + ")");
    if (seen[list[k]]) return fail(fn + ": " + what + " " + std::to_string(list[k]) + " is listed twice");
    seen[list[k]] = 1;
  }
  return 0;
}

template <class B>
int state_capture(Handle<B>* h, uint32_t n, const uint32_t* envs, uint64_t* row_off, uint64_t* cell_off) {
  const std::string fn = "sfl_state_capture";
  if (!row_off || !cell_off) return fail(fn + ": null argument");
  if (int rc = snap_refuse(h, fn)) return rc;
  if (int rc = snap_list(h, fn, "env", n, envs)) return rc;
  if (int rc = snap_tables(h, fn)) return rc;
  typename Handle<B>::Snap& sn = h->snap;
  snap_drop(h);
  SnapArgs& a = sn.a;
  snap_args(h, a, n);
  bool ok = true;
  auto buf = [&](size_t bytes) -> void* {
    void* p = h->be.alloc(bytes ? bytes : 1);
    if (p) sn.bufs.push_back(p);
    ok = ok && p;
    return p;
  };
  uint32_t* d_envs = (uint32_t*)buf((size_t)n * 4);
  a.envs = d_envs;
  a.live = (uint32_t*)buf((size_t)n * a.tw * 4);
  a.grp_rows = (uint32_t*)buf((size_t)n * a.groups * 4);
  a.grp_cells = (uint32_t*)buf((size_t)n * a.groups * 4);
  a.row_off = (uint64_t*)buf(((size_t)n + 1) * 8);
  a.cell_off = (uint64_t*)buf(((size_t)n + 1) * 8);
  if (!ok) {
    snap_drop(h);
    return fail(fn + ": device allocation failed");
  }
  row_off[0] = cell_off[0] = 0;
  float ms = 0.f;
  if (n) {
    h->be.h2d(d_envs, envs, (size_t)n * 4);
    int rc = h->be.snap(a, SNAP_COUNT, &ms);
    if (!rc) {
      h->be.d2h(row_off, a.row_off, ((size_t)n + 1) * 8);
      h->be.d2h(cell_off, a.cell_off, ((size_t)n + 1) * 8);
    }
    if (h->be.sync()) rc = -1;  // (the host source of the env list lives until here)
    if (rc) {
      snap_drop(h);
      return fail(fn + ": " + h->be.error());
    }
  }
  sn.n_rows = row_off[n];
  sn.n_cells = cell_off[n];
  sn.capture_ms = ms;
  sn.pending = true;
  return 0;
}

template <class B>
int state_read(Handle<B>* h, uint8_t* state, uint32_t* touched, uint32_t* row_ids, uint64_t* cells) {
  const std::string fn = "sfl_state_read";
  typename Handle<B>::Snap& sn = h->snap;
  if (!sn.pending) return fail(fn + ": no pending capture (sfl_state_capture)");
  SnapArgs& a = sn.a;
  const size_t n = a.n;
  bool ok = true;
  auto buf = [&](size_t bytes) -> void* {
    void* p = h->be.alloc(bytes ? bytes : 1);
    if (p) sn.bufs.push_back(p);
    ok = ok && p;
    return p;
  };
  a.row_ids = (uint32_t*)buf(sn.n_rows * 4);
  a.cells = (uint64_t*)buf(sn.n_cells * 8);
  a.keys = (uint32_t*)buf(n * a.tw * 4);
  a.state = (uint8_t*)buf(n * a.state_bytes);
  int rc = ok ? 0 : -1;
  float ms = 0.f;
  if (ok && n) {
    h->be.memset(a.state, 0, n * a.state_bytes);  // (the alignment gaps of a record read as zero)
    rc = h->be.snap(a, SNAP_GATHER, &ms);
    if (!rc) {
      if (state) h->be.d2h(state, a.state, n * a.state_bytes);
      if (touched) h->be.d2h(touched, a.keys, n * a.tw * 4);
      if (row_ids && sn.n_rows) h->be.d2h(row_ids, a.row_ids, sn.n_rows * 4);
      if (cells && sn.n_cells) h->be.d2h(cells, a.cells, sn.n_cells * 8);
    }
    if (h->be.sync()) rc = -1;
  }
  snap_drop(h);
  if (!ok) return fail(fn + ": device allocation failed");
  if (rc) return fail(fn + ": " + h->be.error());
  sn.capture_ms += ms;
  return 0;
}

template <class B>
int state_restore(Handle<B>* h, uint64_t fingerprint, uint32_t layout, uint32_t n, const uint32_t* slots,
                  const uint8_t* state, const uint32_t* touched, const uint64_t* row_off, const uint32_t* row_ids,
                  uint64_t n_rows, const uint64_t* cell_off, const uint64_t* cells, uint64_t n_cells) {
  const std::string fn = "sfl_state_restore";
  if (int rc = snap_refuse(h, fn)) return rc;
  const uint32_t mine = h->variant > 0 ? SFL_STATE_WAVE : SFL_STATE_LANE;
  auto cls = [](uint32_t c) { return c == SFL_STATE_WAVE ? "wave" : c == SFL_STATE_LANE ? "lane" : "unknown"; };
  if (layout != mine)
    return fail(fn + ": a record of the " + cls(layout) + " layout class into a handle of the " + cls(mine) +
                " class (records are restored into their own layout class only)");
  if (fingerprint != snap_fingerprint(h))
    return fail(fn + ": fingerprint mismatch: the record was taken with another map, gamma, default_q, ntab, max_steps, "
                     "delay_threshold or malfunction stream than this handle's");
  if (int rc = snap_list(h, fn, "slot", n, slots)) return rc;
  if (n == 0) return 0;
  if (!state || !touched || !row_off || !cell_off || (n_rows && !row_ids) || (n_cells && !cells))
    return fail(fn + ": null argument");
  if (int rc = snap_tables(h, fn)) return rc;
  typename Handle<B>::Snap& sn = h->snap;
  SnapArgs a;
  snap_args(h, a, n);
  if (row_off[0] != 0 || cell_off[0] != 0) return fail(fn + ": row_off / cell_off do not start at 0");
  for (uint32_t k = 0; k < n; ++k)
    if (row_off[k + 1] < row_off[k] || cell_off[k + 1] < cell_off[k])
      return fail(fn + ": row_off / cell_off decrease at record " + std::to_string(k));
  if (row_off[n] != n_rows || cell_off[n] != n_cells)
    return fail(fn + ": row_off / cell_off end at " + std::to_string(row_off[n]) + " rows / " + std::to_string(cell_off[n]) +
                " cells, the buffers hold " + std::to_string(n_rows) + " / " + std::to_string(n_cells));
  std::vector<uint32_t> live((size_t)n * a.tw, 0u);
  for (uint32_t k = 0; k < n; ++k) {
    uint64_t nc = 0;
    for (uint64_t j = row_off[k]; j < row_off[k + 1]; ++j) {
      const uint32_t r = row_ids[j];
      if (r >= a.rows)
        return fail(fn + ": record " + std::to_string(k) + ": row id " + std::to_string(r) + " >= rows_per_env " +
                    std::to_string(a.rows));
      if (j > row_off[k] && r <= row_ids[j - 1])
        return fail(fn + ": record " + std::to_string(k) + ": row ids not strictly ascending (" +
                    std::to_string(row_ids[j - 1]) + " then " + std::to_string(r) + ")");
      live[(size_t)k * a.tw + (r >> 5)] |= 1u << (r & 31u);
      nc += sn.row_w[r];
    }
    if (nc != cell_off[k + 1] - cell_off[k])
      return fail(fn + ": record " + std::to_string(k) + ": " + std::to_string(cell_off[k + 1] - cell_off[k]) +
                  " cells, its rows' widths sum to " + std::to_string(nc));
  }
  // (validated: the first device write follows)
  std::vector<void*> scratch;
  auto up = [&](const void* src, size_t bytes) -> void* {
    void* p = h->be.alloc(bytes ? bytes : 1);
    scratch.push_back(p);
    if (p && bytes && src) h->be.h2d(p, src, bytes);
    return p;
  };
  a.envs = (const uint32_t*)up(slots, (size_t)n * 4);
  a.live = (uint32_t*)up(live.data(), live.size() * 4);
  a.grp_rows = (uint32_t*)up(nullptr, (size_t)n * a.groups * 4);
  a.grp_cells = (uint32_t*)up(nullptr, (size_t)n * a.groups * 4);
  a.row_off = (uint64_t*)up(row_off, ((size_t)n + 1) * 8);
  a.cell_off = (uint64_t*)up(cell_off, ((size_t)n + 1) * 8);
  a.cells = (uint64_t*)up(cells, n_cells * 8);
  a.keys = (uint32_t*)up(touched, (size_t)n * a.tw * 4);
  a.state = (uint8_t*)up(state, (size_t)n * a.state_bytes);
  bool ok = true;
  for (void* p : scratch) ok = ok && p;
  float ms = 0.f;
  int rc = ok ? h->be.snap(a, SNAP_RESTORE, &ms) : -1;
  if (h->be.sync()) rc = -1;  // (the host sources of the uploads live until here)
  for (void* p : scratch) h->be.free(p);
  if (!ok) return fail(fn + ": device allocation failed");
  if (rc) return fail(fn + ": " + h->be.error());
  uint32_t nf = 0, seed_off = 0;
  SnapField f[SNAP_MAX_FIELDS];
  snap_fields(h, f, &nf, &seed_off);
  for (uint32_t k = 0; k < n; ++k) memcpy(&h->seeds[slots[k]], state + (size_t)k * a.state_bytes + seed_off, 8);
  sn.restore_ms = ms;
  return 0;
}

}  // namespace sfl
