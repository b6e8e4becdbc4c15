// extern "C" entry points of include/sfl.h over sfl::Handle<Backend>.
// Included once by each build after `using Backend = ...;`.
#include <vector>

using H = sfl::Handle<Backend>;
static inline H* HH(sfl_handle* h) { return reinterpret_cast<H*>(h); }

// build id (build.py build_id: SHA-1 of the sources, the -D defines and the extra flags), and the
// defines and flags themselves, kept in the file as searchable markers
#ifndef SFL_BUILD_ID
#define SFL_BUILD_ID "0000000000000000000000000000000000000000"
#endif
#ifndef SFL_BUILD_DEFS
#define SFL_BUILD_DEFS ""
#endif
#ifndef SFL_BUILD_FLAGS
#define SFL_BUILD_FLAGS ""
#endif
static const char kBuildMarker[] = "SFL_BUILD_ID:" SFL_BUILD_ID;
__attribute__((used)) static const char kBuildDefs[] = "SFL_BUILD_DEFS:[" SFL_BUILD_DEFS "]";
__attribute__((used)) static const char kBuildFlags[] = "SFL_BUILD_FLAGS:[" SFL_BUILD_FLAGS "]";

extern "C" {

int sfl_abi_version(void) { return SFL_ABI_VERSION; }
const char* sfl_build_id(void) { return kBuildMarker + 13; }
const char* sfl_last_error(void) { return sfl::g_last_error.c_str(); }
int sfl_device_count(int* n) { return Backend::device_count(n); }

int sfl_create(const sfl_map_desc* map, const sfl_hparams* hp, uint32_t n_envs, const uint64_t* env_seeds, int device,
               sfl_handle** out) {
  H* h = nullptr;
  int rc = sfl::create<Backend>(map, hp, n_envs, env_seeds, device, &h);
  if (rc == 0) *out = reinterpret_cast<sfl_handle*>(h);
  return rc;
}

int sfl_create_eval(const sfl_map_desc* map, const sfl_hparams* hp, uint32_t n_envs, const uint64_t* env_seeds, int device,
                    uint32_t n_policies, sfl_handle** out) {
  if (n_policies == 0) return sfl::fail("sfl_create_eval: n_policies must be at least 1");
  H* h = nullptr;
  int rc = sfl::create<Backend>(map, hp, n_envs, env_seeds, device, &h, n_policies);
  if (rc == 0) *out = reinterpret_cast<sfl_handle*>(h);
  return rc;
}

// an evaluation handle (sfl_create_eval) has no learner and no per-env table
static int no_eval(H* h, const char* fn, const char* why) {
  return h->bank.on ? sfl::fail(std::string(fn) + ": an evaluation handle " + why + " (sfl_create_eval)") : 0;
}

int sfl_destroy(sfl_handle* h) {
  delete HH(h);
  return 0;
}

int sfl_learn_begin(sfl_handle* h, const uint64_t* rng_states) {
  if (!h || !rng_states) return sfl::fail("sfl_learn_begin: null argument");
  return sfl::learn_begin(HH(h), rng_states);
}

int sfl_apply_qinit(sfl_handle* h, uint32_t n_rows, const uint32_t* row_port, const uint32_t* row_state,
                    const double* values) {
  if (!h) return sfl::fail("sfl_apply_qinit: null handle");
  if (int rc = no_eval(HH(h), "sfl_apply_qinit", "has no per-env table")) return rc;
  if (HH(h)->part.world) return sfl::part_qinit(HH(h), n_rows, row_port, row_state, values);
  return sfl::apply_qinit(HH(h), n_rows, row_port, row_state, values);
}

int sfl_mark_exploit_done(sfl_handle* h) { return sfl::mark_exploit_done(HH(h)); }

// the launch totals were reduced by check_errors at the end of the run
static int count_launch(H*) { return 0; }

int sfl_learn(sfl_handle* h, sfl_run_args* args) {
  if (!h || !args) return sfl::fail("sfl_learn: null argument");
  H* hh = HH(h);
  if (int rc = no_eval(hh, "sfl_learn", "has no learner")) return rc;
  std::vector<int32_t> ept(hh->E);
  hh->be.d2h(ept.data(), hh->st.ep_t, hh->E * 4);
  hh->be.sync();
  sfl::SflCtl c{};
  c.mode = 0;
  c.exploit_freq = args->exploit_freq;
  c.ep_target = ept[0] + args->n_episodes;
  c.stats_base = ept[0];
  c.dec_budget = 0;
  int rc = sfl::run(hh, c, args);
  if (rc == 0) rc = count_launch(hh);
  if (rc == 0) rc = sfl::curve_skip_to_now(hh);
  return rc;
}

int sfl_test(sfl_handle* h, sfl_run_args* args) {
  if (!h || !args) return sfl::fail("sfl_test: null argument");
  H* hh = HH(h);
  if (int rc0 = no_eval(hh, "sfl_test", "has no per-env table; use sfl_bank_eval")) return rc0;
  int rc = sfl::test_begin(hh);
  if (rc) return rc;
  sfl::SflCtl c{};
  c.mode = 1;
  c.ep_target = args->n_episodes;
  c.dec_budget = 0;
  rc = sfl::run(hh, c, args);
  if (rc == 0) rc = count_launch(hh);
  // leave the env ready for a fresh episode in whichever mode comes next
  std::vector<int32_t> ph(hh->E, sfl::PH_RESET);
  hh->be.h2d(hh->st.phase, ph.data(), hh->E * 4);
  hh->be.sync();
  return rc;
}

int sfl_step(sfl_handle* h, int64_t decisions_per_env, uint64_t* decisions_done, double* kernel_ms) {
  if (!h || decisions_per_env <= 0) return sfl::fail("sfl_step: bad argument");
  H* hh = HH(h);
  if (int rc0 = no_eval(hh, "sfl_step", "has no learner")) return rc0;
  sfl::SflCtl c{};
  c.mode = 0;
  c.exploit_freq = hh->cv.x_on ? hh->cv.x_freq : 0;  // greedy rounds only with an exploit record (sfl_curve_exploit)
  c.ep_target = -1;
  c.dec_budget = decisions_per_env;
  int rc = sfl::run(hh, c, nullptr);
  if (rc == 0) rc = count_launch(hh);
  if (decisions_done) *decisions_done = hh->last_dec;
  if (kernel_ms) *kernel_ms = hh->last_kernel_ms;
  return rc;
}

int sfl_get_q(sfl_handle* h, uint32_t env, double* q, uint32_t* touched) {
  H* hh = HH(h);
  if (int rc = no_eval(hh, "sfl_get_q", "has no per-env table; use sfl_bank_get")) return rc;
  if (env >= hh->E) return sfl::fail("sfl_get_q: env out of range");
  if (hh->part.world) return sfl::fail("sfl_get_q: the handle is graph-partitioned (use sfl_part_get_q)");
  if (q) hh->be.d2h(q, hh->st.lrn.q + (size_t)env * hh->map.lrn.q_per_env, hh->map.lrn.q_per_env * 8);
  if (touched) hh->be.d2h(touched, hh->st.lrn.touched + (size_t)env * hh->map.lrn.touched_words, hh->map.lrn.touched_words * 4);
  return hh->be.sync() ? sfl::fail(hh->be.error()) : 0;
}

int sfl_set_q(sfl_handle* h, uint32_t env, const double* q, const uint32_t* touched) {
  H* hh = HH(h);
  if (int rc = no_eval(hh, "sfl_set_q", "has no per-env table; use sfl_bank_set")) return rc;
  if (env >= hh->E) return sfl::fail("sfl_set_q: env out of range");
  if (hh->part.world) return sfl::fail("sfl_set_q: the handle is graph-partitioned");
  if (q) hh->be.h2d(hh->st.lrn.q + (size_t)env * hh->map.lrn.q_per_env, q, hh->map.lrn.q_per_env * 8);
  if (touched) hh->be.h2d(hh->st.lrn.touched + (size_t)env * hh->map.lrn.touched_words, touched, hh->map.lrn.touched_words * 4);
  return hh->be.sync() ? sfl::fail(hh->be.error()) : 0;
}

int sfl_get_counters(sfl_handle* h, sfl_counters* out) {
  H* hh = HH(h);
  out->decisions = hh->total_dec;
  out->last_launch_decisions = hh->last_dec;
  out->last_launch_ticks = hh->last_ticks;
  out->last_launch_alg_bytes = hh->last_bytes;
  out->last_kernel_ms = hh->last_kernel_ms;
  out->kernel_variant = hh->variant;
  out->group_lanes = hh->variant > 0 ? sfl::kVariants[hh->variant].G : 1;
  return 0;
}

int sfl_env_begin(sfl_handle* h) {
  if (!h) return sfl::fail("sfl_env_begin: null handle");
  return sfl::env_begin(HH(h));
}

int sfl_env_begin_wave(sfl_handle* h) {
  if (!h) return sfl::fail("sfl_env_begin_wave: null handle");
  return sfl::env_begin(HH(h), true);
}

int sfl_env_step(sfl_handle* h, sfl_env_io* io) {
  if (!h) return sfl::fail("sfl_env_step: null handle");
  return sfl::env_step(HH(h), io);
}

int sfl_env_step_dev(sfl_handle* h, const sfl_env_dev_io* io) {
  if (!h) return sfl::fail("sfl_env_step_dev: null handle");
  return sfl::env_step_dev(HH(h), io);
}

int sfl_env_sync(sfl_handle* h) {
  if (!h) return sfl::fail("sfl_env_sync: null handle");
  return sfl::env_sync(HH(h));
}

int sfl_env_trans_begin(sfl_handle* h, const sfl_env_trans_io* io) {
  if (!h) return sfl::fail("sfl_env_trans_begin: null handle");
  return sfl::trans_begin(HH(h), io);
}

int sfl_env_trans_end(sfl_handle* h) {
  if (!h) return sfl::fail("sfl_env_trans_end: null handle");
  return sfl::trans_end(HH(h));
}

int sfl_get_obs_tables(sfl_handle* h, int32_t* switch_rc, int32_t* station_rc) {
  if (!h) return sfl::fail("sfl_get_obs_tables: null handle");
  return sfl::get_obs_tables(HH(h), switch_rc, station_rc);
}

int sfl_get_phase_cycles(sfl_handle* h, uint64_t* cycles, int32_t n) {
  if (!h || !cycles || n < 8) return sfl::fail("sfl_get_phase_cycles: null argument or n < 8");
  H* hh = HH(h);
  hh->be.d2h(cycles, hh->d_phase, 8 * sizeof(uint64_t));
  for (int i = 8; i < n; ++i) cycles[i] = 0;
  return hh->be.sync() ? sfl::fail(hh->be.error()) : 0;
}

int sfl_get_kernel_note(sfl_handle* h, char* buf, int32_t cap) {
  if (!h || !buf || cap < 1) return sfl::fail("sfl_get_kernel_note: null argument");
  const std::string& n = HH(h)->variant_note;
  const size_t k = n.size() < (size_t)cap - 1 ? n.size() : (size_t)cap - 1;
  memcpy(buf, n.data(), k);
  buf[k] = 0;
  return 0;
}

int sfl_get_env_state(sfl_handle* h, uint32_t env, int32_t* elapsed, int32_t* phase, uint64_t* sem, int32_t* tr_pos,
                      uint32_t* tr_bits) {
  H* hh = HH(h);
  if (env >= hh->E) return sfl::fail("sfl_get_env_state: env out of range");
  if (int rc = sfl::part_host_access(hh, false)) return rc;
  const size_t E = hh->E;
  if (elapsed) hh->be.d2h(elapsed, hh->st.elapsed + env, 4);
  if (phase) hh->be.d2h(phase, hh->st.phase + env, 4);
  // layouts: the one-env-per-wave body keeps these arrays env-major ([E][NP], [E][T]), the
  // lane-per-env body env-minor ([NP][E], [T][E])
  const bool env_major = hh->variant > 0;
  const size_t NP = (size_t)hh->map.NP, T = (size_t)hh->map.T;
  if (sem) {
    if (env_major) {  // the wave kernels' 32-bit records, in the 64-bit format of the lane body
      std::vector<uint32_t> w(NP);
      hh->be.d2h(w.data(), (const uint32_t*)hh->st.sem + env * NP, NP * 4);
      if (hh->be.sync()) return sfl::fail(hh->be.error());
      for (size_t p = 0; p < NP; ++p) sem[p] = sfl::wave_rec_to64(w[p]);
    } else
      for (size_t p = 0; p < NP; ++p) hh->be.d2h(sem + p, hh->st.sem + p * E + env, 8);
  }
  if (tr_pos) {
    if (env_major) hh->be.d2h(tr_pos, hh->st.tr_pos + env * T, T * 4);
    else
      for (size_t t = 0; t < T; ++t) hh->be.d2h(tr_pos + t, hh->st.tr_pos + t * E + env, 4);
  }
  if (tr_bits) {
    if (env_major) hh->be.d2h(tr_bits, hh->st.tr_bits + env * T, T * 4);
    else
      for (size_t t = 0; t < T; ++t) hh->be.d2h(tr_bits + t, hh->st.tr_bits + t * E + env, 4);
  }
  return hh->be.sync() ? sfl::fail(hh->be.error()) : 0;
}

int sfl_set_mf_schedule(sfl_handle* h, int32_t steps, const uint8_t* table) {
  if (!h) return sfl::fail("sfl_set_mf_schedule: null handle");
  return sfl::set_mf_schedule(HH(h), steps, table);
}

int sfl_mf_schedule_flatland(const uint32_t* key, int32_t nkey, const int32_t* windows, int32_t n_windows, int32_t T,
                             double prob, int32_t mf_min, int32_t mf_max, int32_t steps, uint8_t* out) {
  if (!key || nkey < 1 || (n_windows > 0 && !windows) || T < 1 || steps < 0 || !out || mf_max < mf_min)
    return sfl::fail("sfl_mf_schedule_flatland: bad argument");
  for (int32_t i = 0; i < n_windows; ++i)
    if (windows[i] < 1) return sfl::fail("sfl_mf_schedule_flatland: a departure window below 1 (randint(0, w) needs w >= 1)");
  if (sfl::mf_schedule_flatland(key, nkey, windows, n_windows, T, prob, mf_min, mf_max, steps, out))
    return sfl::fail("sfl_mf_schedule_flatland: a malfunction of more than 255 steps");
  return 0;
}

// ---- graph-partitioned mode (sfl_part.h) ----
int sfl_part_config(sfl_handle* h, int32_t rank, int32_t world, const int32_t* owner, uint32_t env_base,
                    uint32_t envs_total, uint32_t cap_req, uint32_t cap_upd) {
  if (!h || !owner) return sfl::fail("sfl_part_config: null argument");
  return sfl::part_config(HH(h), rank, world, owner, env_base, envs_total, cap_req, cap_upd);
}

int sfl_part_record_sizes(uint32_t* msg, uint32_t* rep) {
  if (!msg || !rep) return sfl::fail("sfl_part_record_sizes: null argument");
  *msg = sizeof(sfl::PartMsg);
  *rep = sizeof(sfl::PartRep);
  return 0;
}

int sfl_part_begin(sfl_handle* h) { return h ? sfl::part_begin(HH(h)) : sfl::fail("sfl_part_begin: null handle"); }

int sfl_part_local(sfl_handle* h, int64_t decisions_per_env, const void* replies, void* messages, uint64_t* requests_sent) {
  if (!h || !replies || !messages) return sfl::fail("sfl_part_local: null argument");
  return sfl::part_local(HH(h), decisions_per_env, replies, messages, requests_sent);
}

int sfl_part_owner(sfl_handle* h, const void* messages, void* replies) {
  if (!h || !messages || !replies) return sfl::fail("sfl_part_owner: null argument");
  return sfl::part_owner(HH(h), messages, replies);
}

int sfl_part_counts(sfl_handle* h, uint32_t* out, int32_t cap) {
  if (!h || !out) return sfl::fail("sfl_part_counts: null argument");
  return sfl::part_counts(HH(h), out, cap);
}

int sfl_get_sync_count(sfl_handle* h, uint64_t* waits, uint64_t* count_reads) {
  if (!h) return sfl::fail("sfl_get_sync_count: null handle");
  if (waits) *waits = HH(h)->be.n_wait;
  if (count_reads) *count_reads = HH(h)->part_reads;
  return 0;
}

int sfl_part_set_caps(sfl_handle* h, uint32_t k_msg) {
  return h ? sfl::part_set_caps(HH(h), k_msg) : sfl::fail("sfl_part_set_caps: null handle");
}

int sfl_part_set_local_rows(sfl_handle* h, const uint8_t* local_switches) {
  if (!h) return sfl::fail("sfl_part_set_local_rows: null handle");
  return sfl::part_set_local_rows(HH(h), local_switches);
}

int sfl_set_stream(sfl_handle* h, void* stream) {
  if (!h) return sfl::fail("sfl_set_stream: null handle");
  if (HH(h)->be.set_stream(stream)) return sfl::fail(std::string("sfl_set_stream: ") + HH(h)->be.error());
  HH(h)->ext_stream = stream != nullptr;
  return 0;
}

int sfl_part_get_q(sfl_handle* h, uint32_t global_env, double* q, uint32_t* touched) {
  if (!h) return sfl::fail("sfl_part_get_q: null handle");
  if (!HH(h)->part.world) return sfl::fail("sfl_part_get_q: handle not partitioned");
  return sfl::part_get_q(HH(h), global_env, q, touched);
}

int sfl_set_hparam_groups(sfl_handle* h, int32_t n_groups, const sfl_hparam_group* groups, const uint16_t* env_group) {
  if (!h) return sfl::fail("sfl_set_hparam_groups: null handle");
  return sfl::set_hparam_groups(HH(h), n_groups, groups, env_group);
}

uint64_t sfl_episode_seed(uint64_t base, uint64_t k) { return sfl::episode_seed(base, k); }

int sfl_set_seed_schedule(sfl_handle* h, uint32_t pool, uint32_t flags) {
  if (!h) return sfl::fail("sfl_set_seed_schedule: null handle");
  return sfl::set_seed_schedule(HH(h), pool, flags);
}

int sfl_get_seed_schedule(sfl_handle* h, uint32_t* pool, uint32_t* flags) {
  if (!h) return sfl::fail("sfl_get_seed_schedule: null handle");
  return sfl::get_seed_schedule(HH(h), pool, flags);
}

int sfl_get_episode_seeds(sfl_handle* h, uint64_t* out) {
  if (!h) return sfl::fail("sfl_get_episode_seeds: null handle");
  return sfl::get_episode_seeds(HH(h), out);
}

int sfl_consensus(sfl_handle* h, int32_t mode, uint32_t flags, uint32_t n_cohorts, const uint32_t* env_cohort,
                  double* kernel_ms) {
  if (!h) return sfl::fail("sfl_consensus: null handle");
  return sfl::consensus(HH(h), mode, flags, n_cohorts, env_cohort, kernel_ms);
}

int sfl_get_consensus_q(sfl_handle* h, uint32_t cohort, double* q, uint32_t* touched) {
  if (!h) return sfl::fail("sfl_get_consensus_q: null handle");
  return sfl::get_consensus_q(HH(h), cohort, q, touched);
}

int sfl_curve_begin(sfl_handle* h, int32_t bin_episodes, int32_t n_bins, uint32_t n_series, const uint32_t* env_series,
                    int32_t ring_cap) {
  if (!h) return sfl::fail("sfl_curve_begin: null handle");
  return sfl::curve_begin(HH(h), bin_episodes, n_bins, n_series, env_series, ring_cap);
}

int sfl_curve_read(sfl_handle* h, sfl_curve_cell* out) {
  if (!h) return sfl::fail("sfl_curve_read: null handle");
  return sfl::curve_read(HH(h), out);
}

int sfl_curve_episodes(sfl_handle* h, int32_t* out) {
  if (!h) return sfl::fail("sfl_curve_episodes: null handle");
  return sfl::curve_episodes(HH(h), out);
}

int sfl_curve_fold_ms(sfl_handle* h, double* last_ms, double* total_ms) {
  if (!h) return sfl::fail("sfl_curve_fold_ms: null handle");
  if (!HH(h)->cv.on) return sfl::fail("sfl_curve_fold_ms: the handle has no curve (sfl_curve_begin)");
  if (last_ms) *last_ms = HH(h)->cv.last_ms;
  if (total_ms) *total_ms = HH(h)->cv.total_ms;
  return 0;
}

int sfl_curve_exploit(sfl_handle* h, int32_t exploit_freq) {
  if (!h) return sfl::fail("sfl_curve_exploit: null handle");
  return sfl::curve_exploit(HH(h), exploit_freq);
}

int sfl_curve_read_exploit(sfl_handle* h, sfl_curve_xcell* out) {
  if (!h) return sfl::fail("sfl_curve_read_exploit: null handle");
  return sfl::curve_read_exploit(HH(h), out);
}

int sfl_curve_rounds(sfl_handle* h, int32_t* out) {
  if (!h) return sfl::fail("sfl_curve_rounds: null handle");
  return sfl::curve_rounds(HH(h), out);
}

int sfl_curve_exploit_fold_ms(sfl_handle* h, double* last_ms, double* total_ms) {
  if (!h) return sfl::fail("sfl_curve_exploit_fold_ms: null handle");
  if (!HH(h)->cv.x_on) return sfl::fail("sfl_curve_exploit_fold_ms: the handle has no exploit record (sfl_curve_exploit)");
  if (last_ms) *last_ms = HH(h)->cv.x_last_ms;
  if (total_ms) *total_ms = HH(h)->cv.x_total_ms;
  return 0;
}

int sfl_curve_end(sfl_handle* h) {
  if (!h) return sfl::fail("sfl_curve_end: null handle");
  return sfl::curve_end(HH(h));
}

// ---- policy-bank evaluation (sfl_eval.h) ----
int sfl_bank_set(sfl_handle* h, uint32_t p, const double* q, const uint32_t* touched) {
  if (!h) return sfl::fail("sfl_bank_set: null handle");
  return sfl::bank_set(HH(h), p, q, touched);
}

int sfl_bank_get(sfl_handle* h, uint32_t p, double* q, uint32_t* touched) {
  if (!h) return sfl::fail("sfl_bank_get: null handle");
  return sfl::bank_get(HH(h), p, q, touched);
}

int sfl_bank_copy(sfl_handle* h, uint32_t p, sfl_handle* src, int32_t kind, uint32_t index) {
  if (!h) return sfl::fail("sfl_bank_copy: null handle");
  return sfl::bank_copy(HH(h), p, HH(src), kind, index);
}

int sfl_bank_eval(sfl_handle* h, const uint32_t* env_policy, sfl_eval_out* out) {
  if (!h) return sfl::fail("sfl_bank_eval: null handle");
  return sfl::bank_eval(HH(h), env_policy, out);
}

int sfl_bank_read(sfl_handle* h, sfl_eval_cell* out) {
  if (!h) return sfl::fail("sfl_bank_read: null handle");
  return sfl::bank_read(HH(h), out);
}

int sfl_bank_fold_ms(sfl_handle* h, double* last_ms, double* total_ms) {
  if (!h) return sfl::fail("sfl_bank_fold_ms: null handle");
  if (!HH(h)->bank.on) return sfl::fail("sfl_bank_fold_ms: not an evaluation handle (sfl_create_eval)");
  if (last_ms) *last_ms = HH(h)->bank.last_ms;
  if (total_ms) *total_ms = HH(h)->bank.total_ms;
  return 0;
}

// ---- the non-arrival diagnosis of the last evaluation (sfl_diag.h) ----
int sfl_bank_diag(sfl_handle* h, int32_t stall, sfl_diag_out* out) {
  if (!h) return sfl::fail("sfl_bank_diag: null handle");
  return sfl::bank_diag(HH(h), stall, out);
}

int sfl_bank_diag_read(sfl_handle* h, sfl_diag_cell* out) {
  if (!h) return sfl::fail("sfl_bank_diag_read: null handle");
  return sfl::bank_diag_read(HH(h), out);
}

int sfl_bank_diag_hot(sfl_handle* h, uint32_t p, uint32_t* out) {
  if (!h) return sfl::fail("sfl_bank_diag_hot: null handle");
  return sfl::bank_diag_hot(HH(h), p, out);
}

int sfl_bank_diag_ms(sfl_handle* h, double* last_ms, double* total_ms) {
  if (!h) return sfl::fail("sfl_bank_diag_ms: null handle");
  if (!HH(h)->bank.on) return sfl::fail("sfl_bank_diag_ms: not an evaluation handle (sfl_create_eval)");
  if (last_ms) *last_ms = HH(h)->bank.dg_last_ms;
  if (total_ms) *total_ms = HH(h)->bank.dg_total_ms;
  return 0;
}

// ---- episodes recorded on the device (sfl_rec.h) ----
int sfl_bank_record(sfl_handle* h, uint32_t n, const uint32_t* envs, int32_t tick_cap, int32_t dec_cap) {
  if (!h) return sfl::fail("sfl_bank_record: null handle");
  return sfl::bank_record(HH(h), n, envs, tick_cap, dec_cap);
}

int sfl_bank_record_info(sfl_handle* h, sfl_record_info* out) {
  if (!h) return sfl::fail("sfl_bank_record_info: null handle");
  return sfl::bank_record_info(HH(h), out);
}

int sfl_bank_record_counts(sfl_handle* h, int32_t* ticks, int32_t* decisions) {
  if (!h) return sfl::fail("sfl_bank_record_counts: null handle");
  return sfl::bank_record_counts(HH(h), ticks, decisions);
}

int sfl_bank_record_read(sfl_handle* h, uint32_t k, int32_t* cell, uint32_t* bits, int32_t* dec) {
  if (!h) return sfl::fail("sfl_bank_record_read: null handle");
  return sfl::bank_record_read(HH(h), k, cell, bits, dec);
}

int sfl_bank_record_traffic(sfl_handle* h, uint32_t p, sfl_record_traffic* out) {
  if (!h) return sfl::fail("sfl_bank_record_traffic: null handle");
  return sfl::bank_record_traffic(HH(h), p, out);
}

int sfl_bank_record_ms(sfl_handle* h, double* last_ms, double* total_ms) {
  if (!h) return sfl::fail("sfl_bank_record_ms: null handle");
  if (!HH(h)->bank.on) return sfl::fail("sfl_bank_record_ms: not an evaluation handle (sfl_create_eval)");
  if (last_ms) *last_ms = HH(h)->bank.rc_last_ms;
  if (total_ms) *total_ms = HH(h)->bank.rc_total_ms;
  return 0;
}

// ---- suspend and resume (sfl_snap.h) ----
int sfl_state_info(sfl_handle* h, sfl_state_desc* out) {
  if (!h) return sfl::fail("sfl_state_info: null handle");
  return sfl::state_info(HH(h), out);
}

int sfl_state_capture(sfl_handle* h, uint32_t n, const uint32_t* envs, uint64_t* row_off, uint64_t* cell_off) {
  if (!h) return sfl::fail("sfl_state_capture: null handle");
  return sfl::state_capture(HH(h), n, envs, row_off, cell_off);
}

int sfl_state_read(sfl_handle* h, uint8_t* state, uint32_t* touched, uint32_t* row_ids, uint64_t* cells) {
  if (!h) return sfl::fail("sfl_state_read: null handle");
  return sfl::state_read(HH(h), state, touched, row_ids, cells);
}

int sfl_state_restore(sfl_handle* h, uint64_t fingerprint, uint32_t layout, uint32_t n, const uint32_t* slots,
                      const uint8_t* state, const uint32_t* touched, const uint64_t* row_off, const uint32_t* row_ids,
                      uint64_t n_rows, const uint64_t* cell_off, const uint64_t* cells, uint64_t n_cells) {
  if (!h) return sfl::fail("sfl_state_restore: null handle");
  return sfl::state_restore(HH(h), fingerprint, layout, n, slots, state, touched, row_off, row_ids, n_rows, cell_off, cells,
                            n_cells);
}

int sfl_state_ms(sfl_handle* h, double* capture_ms, double* restore_ms) {
  if (!h) return sfl::fail("sfl_state_ms: null handle");
  if (capture_ms) *capture_ms = HH(h)->snap.capture_ms;
  if (restore_ms) *restore_ms = HH(h)->snap.restore_ms;
  return 0;
}

}  // extern "C"
