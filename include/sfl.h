/*
 * sfl.h — C-ABI of the MI355X SwitchFL / network-distributed Q-learning hot path.
 *
 * One handle = one batch of E lock-step SwitchFL environments (all on the same
 * compiled map, each with its own seed, its own tabular Q-table and its own RNG
 * stream) resident in the HBM of one GPU.  Plain pointers and sizes only; no
 * torch types.  Every function returns 0 on success and -1 on failure, with the
 * message in sfl_last_error() (thread-local).  Calls are synchronous: they
 * return after the device work they launched has completed.  One handle is used
 * from one host thread.  Multi-GPU = one process and one handle per device.
 *
 * The interfaces these entry points replace in the reference
 * (AI4REALNET/network-distributed-q-learning):
 *
 *   sfl_create        ASyncSwitchEnv(rail_env, max_steps=...)        switchfl/switch_env.py:605-614
 *                     + DistrQLearning(env, gamma, epsilon, ...)     switchfl/distr_q.py:32-45
 *                     (RailNetwork(rail_env) graph compile is done on the host:
 *                      network-distributed-q-learning_amd/compiler.py)
 *   sfl_learn_begin   rng = np.random.default_rng(self.seed),
 *                     agent_num_interactions = {...: 0}               switchfl/distr_q.py:263, 269
 *   sfl_apply_qinit   DistrQLearning.__init_q_table                  switchfl/distr_q.py:81-181, 299-300
 *   sfl_learn         the episode loop of DistrQLearning.learn        switchfl/distr_q.py:275-366
 *   sfl_test          DistrQLearning.test (greedy episode)           switchfl/distr_q.py:184-241
 *   sfl_step          `decisions` iterations of the agent_iter loop  switchfl/distr_q.py:302-362
 *                     (learning mode, episodes restart as they end; the benchmark step)
 *   sfl_get_q / sfl_set_q   DistrQLearning.q_table / save / load     switchfl/distr_q.py:492-527
 *   sfl_get_counters  timing/progress accumulators                   switchfl/switch_env.py:67-73
 *   sfl_env_begin / sfl_env_step   the AEC protocol with an external learner:
 *                     env.reset / agent_iter / last / step(action) / observe
 *                                                                    switchfl/switch_env.py:93, 616-675
 *                     (driven by any learner, e.g. distr_q.py:302-320)
 *   sfl_env_begin_wave   sfl_env_begin with the env step on the handle's wave kernel (one env per wavefront
 *                     or lane group) instead of the lane-per-env body: same calls, same results
 *   sfl_env_step_dev / sfl_env_sync   the same protocol for a policy on the device: device pointers in and
 *                     out, the observation vector of observer.py:269-308 decoded on the device, queued on the
 *                     caller's stream without a wait (the one call that is not synchronous)
 *   sfl_env_trans_begin / sfl_env_trans_end   the learner's pending updates (update_dict, distr_q.py:322-356)
 *                     kept on the device behind every env step: complete transitions appended to a replay
 *                     ring in device memory
 *   sfl_consensus / sfl_get_consensus_q   no counterpart in the reference, whose learners are one process each:
 *                     the envs' Q-tables merged per cohort on the device (mean of the learned values, or the
 *                     optimistic max of distributed Q-learning), handed back to every member, and one consensus
 *                     table per cohort to evaluate and save (DistrQLearning.q_table / save of the merged learner)
 *   sfl_curve_begin / sfl_curve_read   the per-episode record learn() returns (cum_reward, arrived_trains,
 *                     num_malfunctions, delays: distr_q.py:346-366) for sfl_step, reduced on the device into
 *                     learning curves per episode bin and env series instead of [episode][env] host arrays
 *   sfl_create_eval / sfl_bank_eval   DistrQLearning.load + test (distr_q.py:510-527, 184-241) as eval.py runs them
 *                     (eval.py:85-97), for a bank of tables shared by many seeded envs: one greedy episode per env,
 *                     the per-table arrival statistics reduced on the device
 *   sfl_bank_record / sfl_bank_record_read   DistrQLearning.test(plot=True) and ASyncSwitchEnv.render
 *                     (distr_q.py:216-221): the listed envs' bank episodes recorded on the device, every train after
 *                     every tick and every decision, to be rendered on the host; sfl_bank_record_traffic reduces
 *                     them to per-cell and per-switch traffic counts on the device
 *   sfl_get_phase_cycles  the per-phase time accumulators            switchfl/switch_env.py:67-73
 *                     (flatland_step_time, last_time, action_selection_time, update_time, reset_time ...)
 */
#ifndef SFL_H
#define SFL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFL_ABI_VERSION 9

typedef struct sfl_handle sfl_handle;

/* Compiled map (all arrays are host pointers; the library copies them).
 * Layouts are produced by compiler.py; see DESIGN.md "HBM layout". */
typedef struct {
  int32_t H, W;               /* grid size (square) */
  int32_t S, T, K;            /* switches, trains, distinct target stations */
  int32_t max_episode_steps;  /* Flatland timetable horizon */
  double mf_rate;             /* malfunction rate per train per tick */
  int32_t mf_min, mf_max;     /* malfunction duration bounds */
  uint64_t q_per_env;         /* doubles of compact Q-table per env */
  uint32_t rows_per_env;      /* Q rows per env (key-set bitmap) */
  const uint16_t* grid;       /* [H*W] 16-bit Flatland transitions */
  const int16_t* cell_sw;     /* [H*W] switch index or -1 */
  const uint8_t* sw_np;       /* [S] ports */
  const uint8_t* sw_na;       /* [S] actions incl. STOP */
  const uint8_t* act_src;     /* [S*8] route action -> source port slot */
  const uint8_t* act_dst;     /* [S*8] route action -> destination port slot */
  const uint8_t* act_turn;    /* [S*8] second rail action (1 left, 2 forward, 3 right) */
  const uint8_t* act_j;       /* [S*8] index of the action inside its source slot's compact row */
  const uint8_t* first_other; /* [4S] first action not leaving from this slot */
  const uint8_t* port_side;   /* [4S] map_direction(port) */
  const uint8_t* slot_nroutes;/* [4S] routes leaving from this slot */
  const uint8_t* slot_route_act; /* [4S*4] their action indices */
  const uint8_t* q_w;         /* [4S] compact row width = routes + 1 (STOP) */
  const int16_t* port_nb;     /* [4S] rail neighbour port (global id 4*switch+slot) */
  const int16_t* port_len;    /* [4S] plain cells between the two ports */
  const int16_t* port_unique; /* [4S] unique onward port of a target port, or -1 */
  const uint64_t* q_off;      /* [4S] offset (doubles) of the (switch, in-slot) block */
  const uint32_t* row_base;   /* [4S] first row id of the block */
  const int32_t* dist;        /* [K*H*W*4] distance to station, 0x3FFFFFFF = inf */
  const int32_t* tr_ed;       /* [T] earliest departure */
  const int32_t* tr_la;       /* [T] latest arrival */
  const int32_t* tr_k;        /* [T] target station */
  const int32_t* tr_target;   /* [T] target cell */
  const int32_t* tr_init_cell;/* [T] start cell */
  const int32_t* tr_init_dist;/* [T] cells to the first switch port */
  const int32_t* tr_init_delay; /* [T] delay at reset */
  const uint8_t* tr_init_dir; /* [T] start heading */
  const int16_t* tr_init_port;/* [T] first switch port */
  int32_t delay_threshold;    /* StandardObserver(delay_threshold=...) (observer.py:221, default 20): a train's
                                 delay discretises to 1 while delay <= (latest_arrival - earliest_departure)
                                 * delay_threshold (observer.py:228-244), else 2; |value| <= 65536 */
} sfl_map_desc;

typedef struct {
  double gamma, epsilon, epsilon_decay_rate, lr, lr_decay_rate, default_q;
  int64_t max_steps;          /* ASyncSwitchEnv max_steps (truncation) */
  int32_t ntab;               /* length of the two tables below */
  const double* eps_tab;      /* epsilon * decay**n, Python float arithmetic */
  const double* lr_tab;       /* lr * lr_decay**n */
} sfl_hparams;

typedef struct {
  int32_t n_episodes;         /* episodes to run in this call (learn: learning episodes) */
  int32_t exploit_freq;       /* learn: greedy round before episode t when (t+1) % f == 0 (0 = off) */
  int32_t stats_cap;          /* rows of the output buffers below (>= n_episodes to keep all) */
  int32_t pad_;
  /* optional host outputs, row = episode index % stats_cap, [row][env] ([row][train][env] for delays) */
  double* cum_reward;
  int32_t* arrived;
  int32_t* malfunctions;
  int32_t* decisions;
  int32_t* ticks;
  int32_t* delays;
  double* exploit_cum;
  int32_t* exploit_arrived;
  /* optional per-decision trace of one env (debug / parity tests): [trace_cap][4] uint64 */
  uint64_t* trace;
  uint64_t* trace_n;
  int32_t trace_env;
  int32_t trace_cap;
} sfl_run_args;

typedef struct {
  uint64_t decisions;         /* agent-env-steps over all envs since create */
  uint64_t last_launch_decisions;
  uint64_t last_launch_ticks;
  uint64_t last_launch_alg_bytes; /* sum of 220+48P+8A per decision + 36*T_live per env-tick */
  double last_kernel_ms;      /* device time of the last run/step launch (HIP events) */
  int32_t kernel_variant;     /* 0: one env per lane (k_run); v > 0: one env per lane group (k_wave shape v) */
  int32_t group_lanes;        /* lanes per env */
} sfl_counters;

int sfl_abi_version(void);
/* SHA-1 of the sources the library was built from (build.py kernel_source_sha1); the Python
 * loader refuses a library whose id differs from the sources in its tree (a stale build) */
const char* sfl_build_id(void);
const char* sfl_last_error(void);
int sfl_device_count(int* n);

int sfl_create(const sfl_map_desc* map, const sfl_hparams* hp, uint32_t n_envs, const uint64_t* env_seeds,
               int device, sfl_handle** out);
int sfl_destroy(sfl_handle* h);

int sfl_learn_begin(sfl_handle* h, const uint64_t* rng_states /* [n_envs][5] */);
int sfl_apply_qinit(sfl_handle* h, uint32_t n_rows, const uint32_t* row_port, const uint32_t* row_state,
                    const double* values /* [n_rows][4], NaN = default_q */);
int sfl_mark_exploit_done(sfl_handle* h);
int sfl_learn(sfl_handle* h, sfl_run_args* args);
int sfl_test(sfl_handle* h, sfl_run_args* args);
int sfl_step(sfl_handle* h, int64_t decisions_per_env, uint64_t* decisions_done, double* kernel_ms);

int sfl_get_q(sfl_handle* h, uint32_t env, double* q /* [q_per_env] */, uint32_t* touched /* [(rows+31)/32] */);
int sfl_set_q(sfl_handle* h, uint32_t env, const double* q, const uint32_t* touched);
int sfl_get_counters(sfl_handle* h, sfl_counters* out);
/* why this handle runs the lane-per-env body (kernel_variant 0) instead of the one-env-per-wavefront
 * kernel, e.g. "timetable horizon beyond 8191 ticks"; "" when it runs k_wave or k_run was requested */
int sfl_get_kernel_note(sfl_handle* h, char* buf, int32_t cap);
/* read back one env's state word arrays (debug / parity tests) */
int sfl_get_env_state(sfl_handle* h, uint32_t env, int32_t* elapsed, int32_t* phase, uint64_t* sem /* [4S] */,
                      int32_t* tr_pos /* [T] */, uint32_t* tr_bits /* [T] */);

/* ---- Flatland-compatible malfunction stream ----
 * Replaces the counter-based malfunction draw (the default, oracle/flatland_lite.py mf_draw) with
 * a table of the proposals Flatland's ParamMalfunctionGen draws from the env's np_random each step
 * (flatland.envs.malfunction_generators, built at test_model.py:14-19 / main.py:28-33 and
 * reseeded by RailEnv.reset(random_seed=seed) at switch_env.py:99): table[n_envs][steps][T] =
 * num_broken_steps proposed to train h at step t + 1 of an episode (0 = none); a proposal starts
 * a malfunction only for a train that is not done and not already malfunctioning (the
 * MalfunctionHandler rule).  steps == 0 returns to the counter-based draw. */
int sfl_set_mf_schedule(sfl_handle* h, int32_t steps, const uint8_t* table);
/* Host helper (no device): one env's table from its seeding words (flatland.utils.seeding.np_random:
 * key = the sha512-derived init_by_array words), the timetable's randint(0, window) draws consumed
 * at reset (flatland_patch/timetable_generators.py:115), prob = 1 - exp(-malfunction_rate),
 * durations randint(mf_min, mf_max + 1) + 1.  out[steps][T]. */
int sfl_mf_schedule_flatland(const uint32_t* key, int32_t nkey, const int32_t* windows, int32_t n_windows, int32_t T,
                             double prob, int32_t mf_min, int32_t mf_max, int32_t steps, uint8_t* out);

/* ---- graph-partitioned mode (BASELINE.json configs[4]; SURVEY.md §8(e) "C5") ----
 * The switch agents are partitioned over `world` ranks (owner[S]); rank r stores the Q rows of
 * the switches it owns for all `envs_total` envs of the job, and simulates its own envs
 * [env_base, env_base + n_envs).  A round: sfl_part_local (every local env applies the reply
 * to its last request, runs to its next decision and stages that decision's request, plus the
 * update records of its post step; the staged records are packed into one message segment per
 * destination rank, each env's records for that rank as a contiguous group: its updates in the
 * order it made them, then its request), ONE all-to-all of the message buffer, sfl_part_owner on
 * the received segments (per group: the updates in order, then the answer to the request), and an
 * all-to-all of the replies back.  Buffers are [world][k + 1] records (record 0 of a segment =
 * header holding the count; k = the capacity of sfl_part_set_caps, cap_req + cap_upd until then):
 * messages of sfl_part_record_sizes' `msg` bytes, replies of `rep` bytes, a reply at its request's
 * record index; on the GPU they are device pointers (the caller's RCCL buffers).  An env whose group
 * does not fit this round's segment is deferred whole: it sends nothing (its places below the
 * segment end carry void records), sits out the next sfl_part_local and sends the same records
 * again -- so the exchange has a fixed size and needs no counts, and results do not depend on k.
 * Replaces the reference's in-process successor lookup max_q(next_state, next_agent) and update
 * (switchfl/distr_q.py:419-466) across GPU boundaries. */
int sfl_part_config(sfl_handle* h, int32_t rank, int32_t world, const int32_t* owner /* [S] */, uint32_t env_base,
                    uint32_t envs_total, uint32_t cap_req /* >= n_envs */, uint32_t cap_upd);
int sfl_part_record_sizes(uint32_t* msg, uint32_t* rep);
int sfl_part_begin(sfl_handle* h);  /* start a part step: per-env decision counters to 0 */
/* requests_sent: the envs with a request or deferred this round (null: see sfl_set_stream) */
int sfl_part_local(sfl_handle* h, int64_t decisions_per_env, const void* replies, void* messages,
                   uint64_t* requests_sent /* null: see sfl_set_stream */);
int sfl_part_owner(sfl_handle* h, const void* messages, void* replies);
/* this rank's record counts of the last sfl_part_local: out[0 .. world) message records per
 * destination (staged, sent or deferred); then, when cap allows (2 world + 3 words): out[world .. 2 world)
 * their peaks since the previous call, out[2 world] the envs with a request or deferred, out[2 world + 1]
 * the envs deferred in that round, out[2 world + 2] the deferrals since the previous call.  cap >= world;
 * synchronises if sfl_part_local did not (and reports the envs' errors) */
int sfl_part_counts(sfl_handle* h, uint32_t* out, int32_t cap);
/* the segment capacity of the next rounds (records per destination, 1 <= k <= cap_req + cap_upd):
 * every rank of the job sets the same value, at a point where no round is in flight (the buffers of
 * a round are [world][k + 1] records).  A smaller k moves fewer bytes per round; an env that does not
 * fit waits a round (see above). */
int sfl_part_set_caps(sfl_handle* h, uint32_t k_msg);
/* how often the handle has waited for its device since create (stream / event synchronisations; 0 on
 * the host build) and read the round counts back (sfl_part_counts, sfl_part_local with requests_sent):
 * what a caller checks to see that its rounds queue without the host in the loop */
int sfl_get_sync_count(sfl_handle* h, uint64_t* waits, uint64_t* count_reads);
/* queue the handle's work on the caller's stream (a hipStream_t, e.g. torch's current stream,
 * which its RCCL collectives follow).  Then sfl_part_owner returns without a
 * synchronisation, and so does sfl_part_local when requests_sent is null (its counts are read by
 * sfl_part_counts): the rounds between two sfl_part_counts calls queue without a synchronisation.
 * null: the handle's own stream again; SFL_STREAM_DEFAULT: the device's default stream (whose own handle is
 * the null pointer, e.g. torch's current stream when no other was chosen) */
#define SFL_STREAM_DEFAULT ((void*)1)
int sfl_set_stream(sfl_handle* h, void* stream);
/* Which switches' rows the wave kernel decides on and updates in place: local_switches[S] (1 = in
 * place; only switches this rank owns), null = every switch this rank owns (the default after
 * sfl_part_config).  The other rows travel as requests / update records to their owners -- with
 * one rank and the default, no messages at all.  Marking fewer switches local rehearses a bigger
 * job's message traffic on one rank (all zero: every row operation as a message, like the
 * lane-per-env body).  Results are identical either way. */
int sfl_part_set_local_rows(sfl_handle* h, const uint8_t* local_switches);
/* owned Q blocks of one env of the job, written into the full per-env layout of sfl_get_q
 * (other entries untouched); owned key-set bits OR-ed into touched */
int sfl_part_get_q(sfl_handle* h, uint32_t global_env, double* q, uint32_t* touched);

/* ---- external-action mode: the AEC protocol with the policy / learner on the host ----
 * sfl_env_begin turns the handle into n_envs plain environments (no learner: no epsilon draw, no Q-table
 * access), each at a fresh reset.  Each sfl_env_step call then, per env: applies actions[e] to the
 * observation the previous call emitted (ASyncSwitchEnv.step -> _apply_action, and _move_trains_to_switch
 * when no switch is active: switch_env.py:632-666), and runs on to the env's next decision, whose
 * observation it emits (agent_iter pops it, last() / observe() read it: switch_env.py:616-630, 668-675,
 * observer.py:246-308) -- or reports the episode's end (agent = -1; the next call resets:
 * switch_env.py:93-158).  actions == null (or an action < 0) applies nothing and re-emits the pending
 * observation; SFL_ACTION_RESET resets the env where it stands (env.reset() in the middle of an episode:
 * the same reset as at an episode end, switch_env.py:93-158) and emits the new episode's first observation.
 * An action outside the deciding switch's action space is refused (E_BAD_ACTION, switch_env.py:213-215)
 * without touching the env.  Output arrays are host pointers, [n_envs] unless stated; null skips one. */
#define SFL_ACTION_RESET (-2)
typedef struct {
  const int32_t* actions;  /* in: action for each env's pending observation (< 0 or null: none) */
  int32_t* agent;          /* deciding switch index of the emitted observation; -1: the episode ended */
  int32_t* train;          /* active train (info["active_train"]) */
  int32_t* slot;           /* in-port slot of the active train at the switch */
  uint32_t* state;         /* observation index ((free_port_bits * K + station) * 3 + delay level): the
                              observation vector [r, c, sem[P], target[2P], delay[P]] (observer.py:269-308) */
  uint32_t* mask;          /* info["action_mask"] as bits (bit a: action a allowed) */
  int32_t* reward;         /* last() reward of (agent, train) (switch_env.py:289, AECEnv.last) */
  int32_t* now;            /* rail_env._elapsed_steps at the observation */
  int32_t* next_switch;    /* step() "next_switch" of the applied action (-1: none applied) */
  int32_t* step_now;       /* _elapsed_steps when that step() returned (-1: none applied) */
  uint32_t* arrived;       /* [4][n_envs] arrived-train bitmask ("arrived_trains") after this call */
  int32_t* malfunctions;   /* episode end: num_malfunctions */
  int32_t* delays;         /* episode end: [T][n_envs] train_to_last_node delays */
  int32_t* truncated;      /* episode end: 1 truncation (max_steps), 0 termination */
} sfl_env_io;
int sfl_env_begin(sfl_handle* h);
/* sfl_env_begin with the env step on the wave kernel of the shape the handle was created with (sfl_get_counters:
 * kernel_variant, group_lanes; a handle created on the LDS-map shape steps the same shape without the LDS tables)
 * instead of the lane-per-env body.  Every later call -- sfl_env_step, sfl_env_step_dev, sfl_env_sync,
 * sfl_get_env_state -- is the same and returns the same bits.  Fails, with sfl_get_kernel_note's reason in the
 * message, on a handle without a wave shape (e.g. more than 256 switches, or SFL_KERNEL=scalar) and on a build
 * without wave kernels (the host build).  Either begin call may follow the other on one handle: each starts every
 * env fresh in its own kernel. */
int sfl_env_begin_wave(sfl_handle* h);
int sfl_env_step(sfl_handle* h, sfl_env_io* io);

/* ---- external-action mode with the policy on the device: tensors in and out, no host in the loop ----
 * sfl_env_step_dev is sfl_env_step with every pointer in DEVICE memory (host memory on the host build): per
 * env the same semantics (the action applied to the pending observation, the run to the next decision or the
 * episode end, SFL_ACTION_RESET, a negative or null action re-emitting the pending observation, an action
 * outside the switch's action space refused with E_BAD_ACTION and the observation emitted again).  The call is
 * queued on the handle's current stream (the caller's after sfl_set_stream) and returns without waiting for
 * the device: no stream or event synchronisation and, while the output pointers stay those of the previous call,
 * no copy from host memory (the actions may come from a new buffer every call: they are copied device-to-device,
 * in stream order, into the handle's own).  It returns -1 for argument and launch errors only; the envs' error flags (a
 * refused action) surface at sfl_env_sync, which waits for the stream and reports them as sfl_env_step does.
 * Device steps advance neither sfl_counters.last_kernel_ms nor the decisions counters (they are read on the
 * host).  sfl_env_step and sfl_env_step_dev may be mixed on one handle: both act on the same env state, and
 * a host call with null actions after device calls re-emits the pending observation into host memory.
 *
 * Besides the sfl_env_io fields the device call decodes the observation (observer.py:269-308) on the device:
 * obs[e] = [r, c, sem[4], target[4][2], delay[4]] of the deciding switch, CompiledMap.obs_of_row padded to four
 * ports: obs[0..1] the switch cell, obs[2 + j] sem[j], obs[6 + 2j], obs[7 + 2j] target[j], obs[14 + j] delay[j],
 * all -1 for ports j >= the switch's port count.  When the episode ended in this call (agent == -1) the whole
 * row is -1, the mask row 0, n_actions 0 and done 1.  obs must be 8-byte and action_mask 16-byte aligned. */
#define SFL_OBS_WIDTH 18   /* r, c, sem[4], target[8], delay[4] */
#define SFL_MAX_ACTIONS 16 /* a switch has up to 9 actions (8 routes + STOP); a row is one 16-byte store */
typedef struct {
  sfl_env_io io;         /* the same fields as the host call, but every non-null pointer is DEVICE memory */
  int32_t* obs;          /* [n_envs][SFL_OBS_WIDTH], see above; null skips */
  uint8_t* action_mask;  /* [n_envs][SFL_MAX_ACTIONS], 1 = allowed; null skips */
  int32_t* n_actions;    /* [n_envs] the deciding switch's Discrete(n); 0 when the episode ended */
  uint8_t* done;         /* [n_envs] 1 when agent == -1 (the episode ended in this call) */
} sfl_env_dev_io;
int sfl_env_step_dev(sfl_handle* h, const sfl_env_dev_io* io);
int sfl_env_sync(sfl_handle* h);
/* ---- external-action mode: learner transitions assembled on the device ----
 * A switch's action is credited later: its reward arrives with the next decision of the same train at the successor
 * switch, or as the destination bonus when the train arrives (the reference's update_dict keyed (next_switch, train),
 * distr_q.py:283, 322-356).  Between sfl_env_trans_begin and sfl_env_trans_end that bookkeeping runs on the device
 * behind EVERY sfl_env_step and sfl_env_step_dev of the handle (the two may be mixed), on the same stream, and
 * appends complete transitions to a replay ring the caller owns.  Per env, with (s, h, obs, r, mask) the decision the
 * previous call emitted and a the action this call applied to it (a >= 0, not refused: next_switch >= 0):
 *   1. if (s, h) is pending: the row {the entry's agent, obs, action; reward r; next_agent s, next_obs obs,
 *      next_action_mask mask; terminal 0}, and the entry goes (after a STOP agent == next_agent: emitted like any other);
 *   2. pending[(next_switch, h)] = (s, obs, a)   (an entry already there is overwritten);
 *   3. for each train newly in `arrived`, in ascending order, each of its pending entries in ascending switch order:
 *      the row {the entry's agent, obs, action; reward SFL_DEST_BONUS; next_agent -1, next_obs all -1, mask 0,
 *      next_n_actions 0; terminal 1}, and the entry goes (this covers the entry step 2 just wrote);
 *   4. if the episode ended in this call (agent == -1) or the action is SFL_ACTION_RESET: dropped[e] += the env's
 *      pending entries, and the table empties (after 1-3 at an episode end; alone at a reset).
 * A call that applies nothing to an env (a negative or null action, a refused action, the first call after begin)
 * emits nothing for it.  Rows carry env, train and now of the entry's decision.  Order: calls in order, envs ascending
 * within a call, the order above within an env.  Row g of the run (g = 0, 1, ...) lands in slot g % capacity; of a
 * call with more than `capacity` rows only the last `capacity` are written.  total[0] counts all rows since begin
 * and last_count[0] those of the last call; both live in device memory and are written (never read) by the kernels, so
 * a consumer on the same stream needs no host round trip.  Every pointer is DEVICE memory (host memory on the host
 * build); obs / next_obs / next_action_mask may be null (skipped) and must be 8- / 8- / 16-byte aligned, rows as
 * sfl_env_step_dev's obs and action_mask.  sfl_env_trans_begin zeroes total, last_count and dropped and leaves the
 * columns as they are; it fails on a handle that is not in external-action mode, on an evaluation handle, on a
 * graph-partitioned handle and with capacity 0.  sfl_env_begin / sfl_env_begin_wave end a running assembler. */
#define SFL_DEST_BONUS 1000 /* the learner's destination bonus (distr_q.py destination_bonus) */
typedef struct {
  uint32_t capacity; /* N, rows of the ring (1 .. 2^31 - 1) */
  uint32_t pad_;
  int32_t* env;            /* [N] */
  int32_t* train;          /* [N] */
  int32_t* now;            /* [N] elapsed ticks at the entry's decision */
  int32_t* agent;          /* [N] the deciding switch */
  int32_t* action;         /* [N] */
  int32_t* reward;         /* [N] */
  int32_t* next_agent;     /* [N] -1: terminal */
  int32_t* next_n_actions; /* [N] Discrete(n) of next_agent; 0: terminal */
  uint8_t* terminal;       /* [N] */
  int32_t* obs;            /* [N][SFL_OBS_WIDTH] or null */
  int32_t* next_obs;       /* [N][SFL_OBS_WIDTH] or null */
  uint8_t* next_action_mask; /* [N][SFL_MAX_ACTIONS] or null */
  int64_t* total;          /* [1] */
  int32_t* last_count;     /* [1] */
  int64_t* dropped;        /* [n_envs] */
} sfl_env_trans_io;
int sfl_env_trans_begin(sfl_handle* h, const sfl_env_trans_io* io);
int sfl_env_trans_end(sfl_handle* h);
/* the two coordinate tables the observation decode reads, as derived at sfl_create from cell_sw and from
 * tr_k / tr_target (debug / tests): switch_rc[S][2] and station_rc[K][2] as (row, column); null skips one */
int sfl_get_obs_tables(sfl_handle* h, int32_t* switch_rc, int32_t* station_rc);
/* Device time per phase of the learn loop since create, accumulated from in-kernel cycle counters of a
 * sample of the wavefronts (the kernels with one env per lane group; zero for the lane-per-env body):
 * cycles[0] tick (Flatland RailEnv.step + _move_trains / _check_active_switch), [1] observe (last()),
 * [2] epsilon-greedy action selection, [3] apply (_apply_action), [4] post (Q update, pending map,
 * destination bonus), [5] reset, [6] other (launch state load / store, loop control), [7] the sampled
 * wavefronts' total; their ratios split the launches' kernel time (switch_env.py:67-73 accumulators).
 * n >= 8. */
int sfl_get_phase_cycles(sfl_handle* h, uint64_t* cycles, int32_t n);

/* ---- hyperparameter groups: a whole epsilon / lr grid in one lock-step batch ----
 * The reference sweeps epsilon, epsilon_decay_rate, lr and lr_decay_rate as one process per grid cell
 * (hyperparam_tuning.py -> main.py); here the cells are envs of one handle.  Env e learns with
 * groups[env_group[e]]: its epsilon(n) and lr(n) schedules (distr_q.py:59-79) come from that group's tables and
 * scalars instead of the handle's sfl_hparams.  Only these four keys are per group: gamma, default_q, max_steps
 * and ntab (the length of every group's tables) stay the handle's.  n_groups == 0 returns to the handle's own
 * sfl_hparams.  1 <= n_groups <= 4096, every env_group[e] < n_groups.  The call copies the arrays, is
 * synchronous and takes effect from the next launch.  Refused on a graph-partitioned handle and in
 * external-action mode; on a grouped handle a per-decision trace (sfl_run_args.trace) is refused and the phase
 * cycles do not advance (the grouped kernels are built plain only). */
typedef struct {
  double epsilon, epsilon_decay_rate, lr, lr_decay_rate;
  const double* eps_tab;   /* [ntab of the handle] epsilon * decay**n, host arithmetic */
  const double* lr_tab;    /* [ntab] lr * lr_decay**n */
} sfl_hparam_group;
#define SFL_MAX_HPARAM_GROUPS 4096
int sfl_set_hparam_groups(sfl_handle* h, int32_t n_groups, const sfl_hparam_group* groups,
                          const uint16_t* env_group /* [n_envs] */);

/* ---- seed schedules: a fresh malfunction stream for every episode ----
 * An env's seed keys its malfunction stream (the counter-based draw, oracle/flatland_lite.py mf_draw), and the
 * reference resets every episode with the same one (env.reset(seed=self.seed)): every learning episode, exploit round
 * and test() of an env replays one malfunction realisation.  A seed schedule derives each episode's seed from the
 * env's create-time seed b_e (after sfl_state_restore: the record's) and the episode's index.  THE RULE -- the host
 * build, the kernels, the Python layer and the tests implement it exactly:
 *   sfl_episode_seed(base, k) = base                                                              for k == 0,
 *                             = mix64(base * 0x9E3779B97F4A7C15 + k * 0xD1B54A32D192ED03 + 0x5EED5C4ED01E5EED)  otherwise
 *     (mod 2^64; mix64 as in csrc/sfl_rng.h and oracle/flatland_lite.py).
 *   pool == 1, flags == 0 is the default: every episode runs on b_e, as on a handle that never made the call.
 *   A learning episode with index t -- the env's learning-episode index since sfl_learn_begin, the index curves bin
 *     by -- runs on sfl_episode_seed(b_e, t % pool); with pool == 0 on sfl_episode_seed(b_e, t): no wrap, every
 *     episode new.  Episode 0 always runs on b_e.
 *   A greedy episode -- an exploit round of sfl_learn / sfl_step, or an episode of sfl_test -- runs on b_e (pool index
 *     0, a training scenario), or with SFL_SEED_HELDOUT_EXPLOIT on sfl_episode_seed(b_e, SFL_SEED_HELD_OUT_EPISODE),
 *     which no learning episode uses.  A greedy round does not advance t.
 *   External-action mode: t counts the episodes the env has started since sfl_env_begin / sfl_env_begin_wave, minus
 *     one; an SFL_ACTION_RESET starts a new episode like an episode end does.  No episode is greedy: the flag is refused
 *     in this mode, and so are the begin calls on a handle that has it.  (A first call made after the begin counts
 *     from the call: an env standing at its reset starts episode 0, any other env's episode in flight is episode 0.)
 *   The seed holds for the whole episode: a launch whose decision budget ends inside an episode, or inside an exploit
 *     round, resumes on the same seed.  A call takes effect at each env's next reset.  sfl_learn_begin restarts t at 0.
 *   sfl_get_episode_seeds: per env the seed of the episode it started last (b_e before its first reset).
 *   sfl_state_capture / sfl_state_restore continue bit for bit: the record of a handle that has left the default
 *     carries, behind the fields of every record (the base seed among them), the running episode's seed, and its
 *     fingerprint says so: such records restore into such handles only.  Restore into a handle with the schedule the
 *     record was captured under (runtime.Batch.restore checks it).  Other handles' records and fingerprints are as before.
 * A handle that has left the default launches kernels of its own (also after a return to the default, which they run
 * by the rule); on it a per-decision trace (sfl_run_args.trace) is refused and the phase cycles do not advance, as on
 * a handle with hyperparameter groups.  Refused, with a message and nothing changed: a graph-partitioned handle (and
 * sfl_part_config on a scheduled one); an evaluation handle, whose seeds are chosen at create (derive them with
 * sfl_episode_seed); a handle with a Flatland malfunction table (sfl_set_mf_schedule with steps > 0, and that call on
 * a scheduled handle); pool > 2^31 - 1; unknown flag bits. */
#define SFL_SEED_HELD_OUT_EPISODE 0xFFFFFFFFFFFFFFFFull
#define SFL_SEED_HELDOUT_EXPLOIT  1u
uint64_t sfl_episode_seed(uint64_t base, uint64_t k);
int sfl_set_seed_schedule(sfl_handle* h, uint32_t pool, uint32_t flags);
int sfl_get_seed_schedule(sfl_handle* h, uint32_t* pool, uint32_t* flags);
int sfl_get_episode_seeds(sfl_handle* h, uint64_t* out /* [n_envs] */);

/* ---- consensus Q-tables: a cohort's learners merged on the device, and shared ----
 * The envs of a handle are independent learners.  sfl_consensus merges their Q-tables per cohort -- env e belongs
 * to cohort env_cohort[e] (SFL_NO_COHORT: to none; it is neither read nor written) -- into one consensus table and
 * key set per cohort, which the handle keeps until the next call (sfl_get_consensus_q reads one), and with
 * SFL_CONSENSUS_SHARE writes each cohort's result back into every member.  The rule, exact to the bit (host build,
 * kernels and the test model agree), for cell i of row r of cohort c with members e_0 < e_1 < ...:
 *   holders H: the members whose key-set bit r is set.  Consensus key set: bit r set iff H is not empty.
 *   nobody holds r: the consensus cell is default_q, and SHARE writes no member's cells of that row.
 *   MEAN: contributors C = the holders whose cell differs bitwise from default_q (an env that never updated a cell
 *     does not pull it back toward the default).  C empty: default_q.  All contributors the same bit pattern: that
 *     pattern, no arithmetic (Q-init values survive exactly; a second consensus of a shared cohort changes nothing).
 *     Otherwise total / (double)|C|: the member list is cut by position into chunks of SFL_CONSENSUS_CHUNK, each
 *     chunk's partial starts at +0.0 and adds its contributors in ascending env order, total starts at +0.0 and adds
 *     the partials in ascending chunk order; no FMA.
 *   MAX: over the holders H: the bit pattern of the lowest-indexed holder whose value no other holder exceeds
 *     (compared with >, so -0.0 and +0.0 tie and the lower env wins).
 *   SHARE: every member's cells of held rows become the consensus cells, its key set the OR of its own and the
 *     consensus key set.  Nothing else of an env changes: its interaction counts (the epsilon / lr schedule
 *     position), pending-update slots (they name cell indices), RNG and episode state stay its own.
 * Synchronous, on the handle's stream (sfl_set_stream); kernel_ms (optional): the device time of the call's kernels
 * (0 on the host build).  Refused: mode other than the two, unknown flag bits, n_cohorts == 0 or > n_envs, an
 * env_cohort[e] that is neither < n_cohorts nor SFL_NO_COHORT, a graph-partitioned handle (its tables are owned
 * rows), a handle in external-action mode (it has no learner); sfl_get_consensus_q also before any sfl_consensus and
 * with cohort >= the last call's n_cohorts.  The consensus buffer is reallocated when n_cohorts changes. */
#define SFL_CONSENSUS_MEAN  0
#define SFL_CONSENSUS_MAX   1
#define SFL_CONSENSUS_SHARE 1u            /* flags: write the result back into every member env */
#define SFL_NO_COHORT       0xFFFFFFFFu   /* env_cohort[e]: env e takes no part and is never written */
#define SFL_CONSENSUS_CHUNK 256           /* members per partial sum (fixes the arithmetic, above) */
int sfl_consensus(sfl_handle* h, int32_t mode, uint32_t flags, uint32_t n_cohorts,
                  const uint32_t* env_cohort /* [n_envs], NULL: every env in cohort 0 */,
                  double* kernel_ms /* optional */);
int sfl_get_consensus_q(sfl_handle* h, uint32_t cohort, double* q /* [q_per_env] */,
                        uint32_t* touched /* [(rows+31)/32] */);

/* ---- step-mode learning curves: the episodes sfl_step ends, reduced on the device ----
 * sfl_step reports decisions only; the per-episode record of the reference's learn() (cum_reward, arrived_trains,
 * num_malfunctions, delays: distr_q.py:346-366) exists through sfl_learn alone, as [episode][env] host arrays.  A
 * curve keeps that record for step mode at any batch size: the handle owns a device ring of ring_cap statistics rows
 * per env (the rows every kernel writes at an episode's end, row = episode index % ring_cap), and after every
 * successful sfl_step launch a fold kernel reduces the rows the launch wrote into a table of n_bins x n_series cells.
 *   Bins: episode i of an env (its learning-episode index since sfl_learn_begin, 0-based) falls in bin
 *     min(i / bin_episodes, n_bins - 1): the last bin collects everything beyond.
 *   Series: env e belongs to series env_series[e] < n_series.  With env_series == NULL on a handle with
 *     hyperparameter groups it is the env's group at the time of the call, and n_series must equal the group count;
 *     with NULL on any other handle it is 0.
 *   Empty cells (count == 0): the min fields are INT64_MAX, the max fields INT64_MIN, first_episode INT64_MAX and
 *     last_episode -1.  `lost` alone may be non-zero in such a cell.
 *   Fold, after each launch, for env e with mark b (the episodes accounted for so far) and a = its episode index
 *     now: the episodes max(b, a - ring_cap) .. a - 1 are folded from ring rows i % ring_cap into their cells; the
 *     episodes b .. max(b, a - ring_cap) - 1, whose rows were overwritten, add 1 to `lost` of their own cell and to
 *     nothing else; the mark becomes a.  A launch of D decisions per env ends at most D + 1 episodes of an env
 *     whose episodes make a decision each (the one the previous launch's last decision finished, then one per
 *     decision at the most), so with ring_cap >= D + 1 nothing is lost; an episode in which no train reaches a
 *     switch makes no decision and is the one way past that bound.  Every field is an integer (cum_reward is an
 *     exact integer in its double), so the table does not depend on the order in which envs are folded.
 *   sfl_curve_begin starts a curve (replacing the handle's curve if it has one): cells empty, every env's mark at
 *     its current episode index (0 right after sfl_learn_begin).  sfl_learn_begin on a handle with a curve zeroes
 *     the marks and empties the cells.  sfl_learn and sfl_test neither record nor fold (their own buffers receive
 *     the rows, as without a curve); after sfl_learn the marks are set to the envs' episode indices, so a later
 *     sfl_step folds only its own episodes.  A handle without a curve runs sfl_step exactly as before.
 *   sfl_curve_read copies the table, [n_bins][n_series] cells; sfl_curve_episodes the marks (per env: the episode
 *     index up to which its learning episodes are accounted for -- folded, lost, or ended before the curve began);
 *     sfl_curve_fold_ms the device time of the last fold and of all folds since sfl_curve_begin (0 on the host
 *     build; never part of sfl_counters.last_kernel_ms or sfl_step's kernel_ms); sfl_curve_end frees everything.
 * Refused: bin_episodes, n_bins, n_series or ring_cap below 1, an env_series[e] >= n_series, n_series other than
 * the group count (NULL series on a grouped handle), a graph-partitioned handle, a handle in external-action mode,
 * a table above SFL_CURVE_MAX_TABLE_BYTES or a ring (ring_cap * n_envs * (24 + 4 T) bytes) above
 * SFL_CURVE_MAX_RING_BYTES; read / episodes / end on a handle without a curve. */
typedef struct {            /* one (bin, series) cell: 16 x int64, 128 bytes */
  int64_t count;            /* episodes folded */
  int64_t lost;             /* episodes that ended but were overwritten in the ring before the fold */
  int64_t arrived_sum, arrived_min, arrived_max;
  int64_t all_arrived;      /* episodes with arrived == T */
  int64_t reward_sum, reward_min, reward_max;   /* cum_reward, an exact integer */
  int64_t decisions_sum, ticks_sum, malfunctions_sum;
  int64_t delay_sum;        /* sum over the episode's T trains of their delays */
  int64_t truncated;        /* episodes with decisions > max_steps */
  int64_t first_episode, last_episode;          /* lowest / highest episode index folded */
} sfl_curve_cell;
#define SFL_CURVE_MAX_TABLE_BYTES (64ull << 20)
#define SFL_CURVE_MAX_RING_BYTES  (1ull << 30)
int sfl_curve_begin(sfl_handle* h, int32_t bin_episodes, int32_t n_bins, uint32_t n_series,
                    const uint32_t* env_series /* [n_envs] or NULL */, int32_t ring_cap);
int sfl_curve_read(sfl_handle* h, sfl_curve_cell* out /* [n_bins][n_series] */);
int sfl_curve_episodes(sfl_handle* h, int32_t* out /* [n_envs] */);
int sfl_curve_fold_ms(sfl_handle* h, double* last_ms, double* total_ms /* either may be NULL */);
int sfl_curve_end(sfl_handle* h);

/* ---- the exploit record of a curve: the greedy rounds sfl_step runs, folded on the device ----
 * The reference judges a learner by its exploit rounds: before learning episode t with (t + 1) % exploit_freq == 0 it
 * runs one greedy episode (distr_q.py:278-281).  sfl_curve_exploit(h, f) with f >= 1 makes every later sfl_step launch
 * with exploit_freq = f -- the kernels then walk the trajectory of sfl_learn with that frequency, a decision budget
 * that runs out inside a round resumes in it -- and record each round's cum_reward and arrived trains in two more
 * arrays of the curve's ring, [ring_cap][n_envs] double and int32 (row = t % ring_cap; 12 more bytes per row and env).
 * Behind the curve's fold a second kernel folds the rounds into a table of n_bins x n_series exploit cells, with the
 * curve's bins and series.  All arithmetic is integer:
 *   Rounds: round r (0-based) of an env precedes episode t_r = (r + 1) * f - 1.  An env at episode index a whose
 *     flags word says "exploit round done" (x) has completed n = a / f + ((x && (a + 1) % f == 0) ? 1 : 0) rounds.
 *   Period: p = ring_cap / gcd(ring_cap, f); rounds r and r + p share a ring row.
 *   Fold, after each launch, for env e with mark b (the rounds accounted for so far): the rounds max(b, n - p) .. n - 1
 *     are folded from ring rows t_r % ring_cap into cell (min(t_r / bin_episodes, n_bins - 1), series[e]): count += 1,
 *     the arrived fields from the row's arrived trains, all_arrived += (arrived == T), the reward fields from
 *     (int64)cum_reward, first_episode / last_episode from t_r.  The rounds b .. max(b, n - p) - 1 add 1 to `lost` of
 *     their own cell and to nothing else.  The mark becomes n.  With ring_cap coprime to f, p = ring_cap, and a launch
 *     of D decisions per env with ring_cap >= D + 1 loses no round.
 *   Empty cells are as in sfl_curve_cell: min fields INT64_MAX, max fields INT64_MIN, first_episode INT64_MAX,
 *     last_episode -1.
 *   sfl_curve_exploit with f >= 1 needs a curve; the first such call allocates the record; every such call empties the
 *     exploit cells and sets each env's mark to the rounds it has completed under f by now.  f == 0: no new round
 *     starts; a round in flight is finished by the kernels (the env's greedy flag holds until its next reset) and
 *     folded, no other round is counted from then on, and the cells stay readable (on a curve without a record the
 *     call does nothing).  sfl_curve_begin on a handle with an exploit record drops it with the curve it replaces;
 *     sfl_curve_end frees it.  sfl_learn_begin empties the cells and zeroes the marks.  sfl_learn and sfl_test neither
 *     record nor fold into it; after sfl_learn and after sfl_mark_exploit_done (which sets the done flag without a
 *     row having been written) the marks are set to the rounds completed now.  A handle on which sfl_curve_exploit
 *     is never called runs sfl_step with exploit_freq = 0 and folds exactly as before.
 *   Not the reference's: with f == 1 an env standing at episode 0 runs its first round on the initialised Q-table
 *     (learn() runs it before __init_q_table, distr_q.py:278-300).  Greedy decisions count towards sfl_step's decisions
 *     per env and the handle's counters, as in sfl_learn.
 *   sfl_curve_read_exploit copies the cells, [n_bins][n_series]; sfl_curve_rounds the marks, [n_envs].  The exploit
 *     fold's device time is part of what sfl_curve_fold_ms reports; sfl_curve_exploit_fold_ms reports it alone.
 * Refused: f < 0; a handle without a curve; a ring whose bytes with the two arrays, ring_cap * n_envs * (36 + 4 T),
 * exceed SFL_CURVE_MAX_RING_BYTES; read_exploit / rounds / exploit_fold_ms on a handle without an exploit record. */
typedef struct {            /* one (bin, series) exploit cell: 11 x int64 */
  int64_t count;            /* rounds folded */
  int64_t lost;             /* rounds that ended but were overwritten in the ring before the fold */
  int64_t arrived_sum, arrived_min, arrived_max;
  int64_t all_arrived;      /* rounds with arrived == T */
  int64_t reward_sum, reward_min, reward_max;   /* cum_reward, an exact integer */
  int64_t first_episode, last_episode;          /* lowest / highest episode index t a folded round preceded */
} sfl_curve_xcell;
int sfl_curve_exploit(sfl_handle* h, int32_t exploit_freq);
int sfl_curve_read_exploit(sfl_handle* h, sfl_curve_xcell* out /* [n_bins][n_series] */);
int sfl_curve_rounds(sfl_handle* h, int32_t* out /* [n_envs] */);
int sfl_curve_exploit_fold_ms(sfl_handle* h, double* last_ms, double* total_ms /* either may be NULL */);

/* ---- policy-bank evaluation: P shared Q-tables, one greedy episode per env, reduced on the device ----
 * The reference evaluates a trained table with DistrQLearning.test (distr_q.py:184-241) in a one-env process, a few
 * runs per experiment (eval.py:85-97).  sfl_test does the same per env of a handle, but every env carries a private
 * copy of its table.  An evaluation handle (sfl_create_eval) instead owns a read-only bank of n_policies tables, each
 * in the layout of sfl_get_q; sfl_bank_eval runs one greedy episode per env, env e on table env_policy[e] and on its
 * own seed, and reduces the episodes into one sfl_eval_cell per table on the device.
 *   sfl_create_eval allocates what sfl_create does except the per-env Q block and key set, plus the bank:
 *     [n_policies][q_per_env] doubles and [n_policies][touched_words] words.  Every table starts as default_q with an
 *     empty key set and counts as unset until sfl_bank_set or sfl_bank_copy fills it.  The kernel is chosen as in
 *     sfl_create (SFL_WAVE_G, SFL_LDS_MAP, SFL_KERNEL; sfl_get_kernel_note); the row with the map tables in LDS runs
 *     its own evaluation kernel (a launch is a whole episode).  hp's epsilon / lr keys are unused.  n_policies == 0
 *     is refused.
 *   sfl_bank_set / sfl_bank_get move table p between host and device (q or touched may be NULL to skip one);
 *     sfl_bank_copy copies device to device from a training handle on the same device: kind SFL_BANK_FROM_ENV env
 *     `index`'s table and key set, SFL_BANK_FROM_COHORT consensus cohort `index`'s (sfl_consensus).  Refused when
 *     q_per_env, rows_per_env or default_q differ, the devices differ, src is an evaluation handle or
 *     graph-partitioned, or there is no such env / cohort.
 *   sfl_bank_eval starts every env from a reset, so a second call replays the same episodes unless the tables or
 *     env_policy changed.  Every pointer of sfl_eval_out is an optional host array.  Refused when an entry of
 *     env_policy is >= n_policies or names a table that was never set.  The handle's counters (sfl_get_counters)
 *     report the launch's decisions, ticks and kernel ms.
 *   The bank is READ-ONLY during an evaluation.  The reference's test() adds every row it looks up to the Q dict
 *     (max_action's __check_entry, and so does sfl_test to the env's key set); sfl_bank_eval records none: the key
 *     sets stay as they were set.  A compact row outside a key set already holds default_q, so the greedy choice, and
 *     with it every output, is the same as sfl_test's on a private copy of the table.
 *   sfl_bank_read: the cells of the last sfl_bank_eval, [n_policies] (refused before the first successful one).
 *     Every field is an integer (cum_reward is an exact integer in its double), so a cell does not depend on the
 *     order the envs were folded in.  The per-train
 *     rule is the train-arrival table's of the reference's notebook (plot.ipynb cell 15), by train handle: at its
 *     destination (at_dest) with delay <= 0 is early, at its destination with delay > 0 late, anything else not
 *     arrived; a train that did not arrive carries a delay too, which is not part of delay_sum_arrived.  (`arrived`,
 *     the reference's arrived_trains counter, is counted at the switches and can be below the at_dest count.)
 *     A table no env followed has episodes == 0, its min fields INT64_MAX and its max fields INT64_MIN.
 *   sfl_bank_fold_ms: the device time of the last fold and of all folds since create (0 on the host build; never
 *     part of sfl_counters.last_kernel_ms).
 *   An evaluation handle has no learner and no per-env table: sfl_learn_begin, sfl_apply_qinit, sfl_learn, sfl_test,
 *     sfl_step, sfl_get_q, sfl_set_q, sfl_consensus, sfl_curve_begin, sfl_part_config, sfl_env_begin /
 *     sfl_env_begin_wave and sfl_set_hparam_groups fail on it with "evaluation handle" in the message.
 *     sfl_get_env_state, sfl_get_counters, sfl_get_kernel_note, sfl_set_mf_schedule and sfl_set_stream work as on any
 *     handle. */
typedef struct {            /* one policy's cell: 15 x int64 */
  int64_t episodes;         /* envs that followed the table in the last sfl_bank_eval */
  int64_t trains_early, trains_late, trains_not_arrived;   /* over those episodes' T trains each */
  int64_t arrived_min, arrived_max;
  int64_t all_arrived;      /* episodes with arrived == T */
  int64_t reward_sum, reward_min, reward_max;   /* cum_reward, an exact integer */
  int64_t decisions_sum, ticks_sum, malfunctions_sum;
  int64_t delay_sum_arrived;  /* sum of the delays of the trains that arrived */
  int64_t truncated;        /* episodes with decisions > max_steps */
} sfl_eval_cell;
typedef struct {            /* optional host outputs of sfl_bank_eval */
  double* cum_reward;       /* [n_envs] */
  int32_t* arrived;         /* [n_envs] */
  int32_t* malfunctions;    /* [n_envs] */
  int32_t* decisions;       /* [n_envs] */
  int32_t* ticks;           /* [n_envs] */
  int32_t* truncated;       /* [n_envs] 1: the episode ended by max_steps */
  int32_t* delays;          /* [T][n_envs] train_to_last_node delays */
  uint8_t* at_dest;         /* [T][n_envs] 1: the train stands at its destination at the episode's end (its state is
                               DONE): the trains_at_dest the reference's test() saves (distr_q.py:237-239) */
} sfl_eval_out;
#define SFL_BANK_FROM_ENV    0
#define SFL_BANK_FROM_COHORT 1
int sfl_create_eval(const sfl_map_desc* map, const sfl_hparams* hp, uint32_t n_envs, const uint64_t* env_seeds,
                    int device, uint32_t n_policies, sfl_handle** out);
int sfl_bank_set(sfl_handle* h, uint32_t p, const double* q /* [q_per_env] */, const uint32_t* touched);
int sfl_bank_get(sfl_handle* h, uint32_t p, double* q, uint32_t* touched);
int sfl_bank_copy(sfl_handle* h, uint32_t p, sfl_handle* src, int32_t kind, uint32_t index);
int sfl_bank_eval(sfl_handle* h, const uint32_t* env_policy /* [n_envs] */, sfl_eval_out* out /* may be NULL */);
int sfl_bank_read(sfl_handle* h, sfl_eval_cell* out /* [n_policies] */);
int sfl_bank_fold_ms(sfl_handle* h, double* last_ms, double* total_ms /* either may be NULL */);

/* ---- policy-bank evaluation: every non-arrival classified on the device ----
 * sfl_bank_eval says per train early, late or not arrived.  sfl_bank_diag says why a train did not arrive, with the
 * classes of scripts/diagnose_nonarrivals.py (its `deadlock` split into queue and cycle), for every episode of the last
 * sfl_bank_eval, from what that launch left on the device: each train's final cell, heading and state, and the tick
 * of its last move, which the bank episode records.  THE RULE -- the host build, the kernels of sfl_diag.hip and the
 * tests' restatement on the Python oracle implement it exactly; every word is an integer, nothing has a tolerance.
 * For env e after its bank episode:
 *   n            the episode's tick count (sfl_eval_out.ticks).
 *   pos_i(h)     train h's cell after tick i; off the map is a value of its own, and pos_0 is off the map.
 *   L(h)         the largest i in 1..n with pos_i(h) != pos_{i-1}(h), or 0 if there is none.
 *   stalled_for(h) = n - L(h) for a train that is on the map at the end, and -1 otherwise.
 *   stalled      on the map at the end and stalled_for(h) >= min(stall, n) - 1: the train's position after each of the
 *                last `stall` ticks equals its final position (the script's window).
 *   blocker(h)   for a stalled train: take MOVE_FORWARD, MOVE_LEFT, MOVE_RIGHT in that order; for each action that is
 *                valid from the train's final (cell, heading) (move_tab: transition valid and new cell valid) take the
 *                cell it leads to and the train with the highest handle that stands on it; if that train is stalled it
 *                is blocker(h) and the search stops.  Otherwise, and for every train that is not stalled, -1.
 *   on a cycle   stalled, and following blocker from h returns to h within T steps.
 *   class, first match wins:
 *     0 SFL_DIAG_ARRIVED         state DONE
 *     1 SFL_DIAG_TRUNCATED       the episode was cut by max_steps (sfl_eval_out.truncated)
 *     2 SFL_DIAG_NEVER_DEPARTED  off the map at the end
 *     3 SFL_DIAG_MOVING_LATE     on the map, not stalled
 *     4 SFL_DIAG_STOP_LOOP       stalled, blocker -1
 *     5 SFL_DIAG_DEADLOCK_QUEUE  stalled, has a blocker, not on a cycle
 *     6 SFL_DIAG_DEADLOCK_CYCLE  stalled, has a blocker, on a cycle
 *   A train stalled in state MALFUNCTION is classified like any other stalled train and counted in a word of its own.
 *   stalled_for, stalled and blocker do not depend on the class: a stalled train of a truncated episode has them too.
 * sfl_diag_cell, per policy, over the episodes that followed it: the trains of classes 1 - 6 (the six class words and
 *   the arrived trains sum to episodes * T); cycles: the trains of class 6 whose handle is the smallest of their cycle,
 *   that is the distinct cycles; episodes_jammed: the episodes with a train of class 5 or 6; stalled_in_malfunction: the
 *   stalled trains whose state is MALFUNCTION; stalled_for_sum / _max over the stalled trains (max: INT64_MIN if none).
 * sfl_bank_diag classifies with the window `stall` (>= 1), on the handle's stream behind the evaluation; it may be
 *   called again with another `stall` without a new evaluation, and changes no output of sfl_bank_eval and no env
 *   state.  Every pointer of sfl_diag_out is an optional host array.  sfl_bank_diag_read: the cells of the last
 *   sfl_bank_diag.  sfl_bank_diag_hot: per cell of the map, the trains of classes 4 - 6 of policy p's episodes that
 *   stand on it.  sfl_bank_diag_ms: the device time of the last diagnosis and of all since create (0 on the host build;
 *   never part of sfl_counters.last_kernel_ms).
 * Refused, with a message in sfl_last_error and the handle usable: a handle that is no evaluation handle; no successful
 *   sfl_bank_eval yet; stall < 1; p >= n_policies; sfl_bank_diag_read / sfl_bank_diag_hot before a successful
 *   sfl_bank_diag of the last evaluation. */
#define SFL_DIAG_ARRIVED         0
#define SFL_DIAG_TRUNCATED       1
#define SFL_DIAG_NEVER_DEPARTED  2
#define SFL_DIAG_MOVING_LATE     3
#define SFL_DIAG_STOP_LOOP       4
#define SFL_DIAG_DEADLOCK_QUEUE  5
#define SFL_DIAG_DEADLOCK_CYCLE  6
typedef struct {            /* one policy's cell: 12 x int64 */
  int64_t episodes;         /* envs that followed the table in the diagnosed sfl_bank_eval */
  int64_t truncated, never_departed, moving_late, stop_loop, deadlock_queue, deadlock_cycle;  /* trains of classes 1 - 6 */
  int64_t cycles;
  int64_t episodes_jammed;
  int64_t stalled_in_malfunction;
  int64_t stalled_for_sum, stalled_for_max;
} sfl_diag_cell;
typedef struct {            /* optional host outputs of sfl_bank_diag */
  uint8_t* cls;             /* [T][n_envs] SFL_DIAG_* */
  int16_t* blocker;         /* [T][n_envs] train handle or -1 */
  int32_t* stalled_for;     /* [T][n_envs] */
} sfl_diag_out;
int sfl_bank_diag(sfl_handle* h, int32_t stall, sfl_diag_out* out /* may be NULL */);
int sfl_bank_diag_read(sfl_handle* h, sfl_diag_cell* out /* [n_policies] */);
int sfl_bank_diag_hot(sfl_handle* h, uint32_t p, uint32_t* out /* [H*W] */);
int sfl_bank_diag_ms(sfl_handle* h, double* last_ms, double* total_ms /* either may be NULL */);

/* ---- policy-bank evaluation: episodes recorded on the device ----
 * sfl_bank_diag names the class of a train that did not arrive; a recording shows the episode that led there: every
 * train after every tick, and every decision.  sfl_bank_eval starts every env from a reset and replays the same
 * episode, so a second evaluation with the jammed envs recorded shows exactly the episodes the diagnosis classified.
 * THE RULE -- the host build and the kernels implement it exactly; every word is an integer, nothing has a tolerance.
 * sfl_bank_record(h, n, envs, tick_cap, dec_cap) arms a recording of the n listed envs (distinct, any order; slot k is
 * envs[k]) on an evaluation handle; an armed recording is replaced, n == 0 disarms and frees it.  Every later
 * sfl_bank_eval then records, for slot k, from the one greedy episode of env e = envs[k]:
 *   frames     after each Flatland tick t = 1 .. min(ticks, tick_cap) of the episode, for every train h:
 *                cell[k][t-1][h]   int32: the train's cell r * W + c after the tick, -1 off the map;
 *                bits[k][t-1][h]   uint32: the train's state word after the tick -- heading in bits 0-1, train state in
 *                                  bits 2-4 (0 WAITING, 1 READY_TO_DEPART, 2 MALFUNCTION_OFF_MAP, 3 MOVING, 4 STOPPED,
 *                                  5 MALFUNCTION, 6 DONE), malfunction counter in bits 13-20, every other bit 0.
 *              The first tick_cap ticks are kept, later ones dropped.
 *   decisions  one row of SFL_REC_DEC_WORDS int32 per decision d = 0 .. min(decisions, dec_cap) - 1, in the order
 *              SFL_REC_NOW .. SFL_REC_STEP_NOW: now, switch, train, slot, state, mask, action, reward, next_switch,
 *              step_now, with the meanings of the same-named sfl_env_io fields (switch: its `agent`): now is
 *              _elapsed_steps when the decision was observed, step_now when its step() returned (the ticks that follow
 *              the last decision of a batch lie between the two).  A truncated episode has max_steps + 1 decisions.
 *   counts     the episode's true ticks and decisions (sfl_eval_out.ticks / .decisions of env e): a slot is complete when
 *              ticks <= tick_cap and decisions <= dec_cap.  Words past the kept frames and rows mean nothing.
 * The buffers belong to the handle: n * (tick_cap * T * 8 + dec_cap * 4 * SFL_REC_DEC_WORDS) bytes, at most
 *   SFL_REC_MAX_BYTES.  A recording changes no output of sfl_bank_eval or sfl_bank_diag* and no env's end state; with
 *   none armed an evaluation on the wave kernels launches kernels that hold none of the recording's code (the recording
 *   kernels are instantiations of their own, launched only while one is armed), and the lane-per-env body and the host
 *   build test one null pointer per tick and decision; nothing more is written either way.
 * Readers, synchronous on the handle's stream: sfl_bank_record_info (n, the caps, the row's word count; n = 0: none
 *   armed); sfl_bank_record_counts ([n] ticks, [n] decisions); sfl_bank_record_read (slot k's arrays, [tick_cap][T],
 *   [tick_cap][T], [dec_cap][SFL_REC_DEC_WORDS]; a NULL pointer skips one).
 * sfl_bank_record_traffic(h, p, out) reduces, on the device, the kept frames and rows of the slots whose env followed
 *   policy p in the last evaluation -- the while-it-happens companion of sfl_bank_diag_hot, which sees final cells only:
 *     occupancy[H*W]              train-ticks on each cell (kept frames with cell >= 0);
 *     standing[H*W]               those whose train held the same cell one tick earlier (frame t-1 against t-2; the
 *                                 frame of tick 1 never counts: every train is off the map before it);
 *     standing_malfunction[H*W]   the part of standing where the train's state after the tick is MALFUNCTION;
 *     decisions[S]                kept rows per switch;     stops[S]   those whose action is the switch's STOP (its last).
 *   All integer sums: the order of the fold does not matter.  Every pointer of sfl_record_traffic is an optional host
 *   array.  sfl_bank_record_ms: the device time of the last traffic fold and of all since create (0 on the host build).
 * Refused, with a message in sfl_last_error and the handle usable: a handle that is no evaluation handle; an env >=
 *   n_envs or listed twice; a cap < 1; a size over SFL_REC_MAX_BYTES; a reader (counts, read, traffic) with no recording
 *   armed or before a successful sfl_bank_eval that followed the arming; k >= n; p >= n_policies. */
#define SFL_REC_DEC_WORDS    10
#define SFL_REC_MAX_BYTES    (1ull << 30)
#define SFL_REC_NOW          0
#define SFL_REC_SWITCH       1
#define SFL_REC_TRAIN        2
#define SFL_REC_SLOT         3
#define SFL_REC_STATE        4
#define SFL_REC_MASK         5
#define SFL_REC_ACTION       6
#define SFL_REC_REWARD       7
#define SFL_REC_NEXT_SWITCH  8
#define SFL_REC_STEP_NOW     9
typedef struct {            /* what sfl_bank_record_info reports */
  uint32_t n;               /* recorded envs (0: no recording armed) */
  int32_t tick_cap, dec_cap;
  uint32_t dec_words;       /* SFL_REC_DEC_WORDS */
} sfl_record_info;
typedef struct {            /* optional host outputs of sfl_bank_record_traffic */
  uint32_t* occupancy;             /* [H*W] */
  uint32_t* standing;              /* [H*W] */
  uint32_t* standing_malfunction;  /* [H*W] */
  uint32_t* decisions;             /* [S] */
  uint32_t* stops;                 /* [S] */
} sfl_record_traffic;
int sfl_bank_record(sfl_handle* h, uint32_t n, const uint32_t* envs /* [n] */, int32_t tick_cap, int32_t dec_cap);
int sfl_bank_record_info(sfl_handle* h, sfl_record_info* out);
int sfl_bank_record_counts(sfl_handle* h, int32_t* ticks /* [n] */, int32_t* decisions /* [n]; either may be NULL */);
int sfl_bank_record_read(sfl_handle* h, uint32_t k, int32_t* cell, uint32_t* bits, int32_t* dec /* any may be NULL */);
int sfl_bank_record_traffic(sfl_handle* h, uint32_t p, sfl_record_traffic* out);
int sfl_bank_record_ms(sfl_handle* h, double* last_ms, double* total_ms /* either may be NULL */);

/* ---- suspend and resume: a batch's state and its live Q rows, packed on the device ----
 * Everything a launch leaves behind is the per-env state, the key set and the Q block of each env.  A capture of n
 * listed envs takes, per env in list order: one state record of state_bytes bytes; the key set ([touched_words]
 * words, as stored); and only the LIVE rows of its Q block.  Row r of an env is live when its key-set bit is set or
 * any of its cells differs from default_q as a 64-bit pattern (-0.0 under default_q = 0.0 is live; so is a NaN).
 *   row_ids[row_off[k] .. row_off[k + 1]): the live rows of the k-th listed env, ascending.
 *   cells[cell_off[k] .. cell_off[k + 1]): their cells as bit patterns, rows in row_ids order, a row's q_w cells in
 *     stored order.
 *   A state record: the env's slice of every per-env state array except the Q block and the key set, in a fixed
 *     order, each array at an offset aligned to its element size, the record padded to a multiple of 8 bytes.  It
 *     holds the env's seed (a uint64 at seed_offset), its epsilon-greedy stream, its interaction counts (the schedule
 *     position), the pending-update slots and the episode state.  Its byte layout depends on the layout class of the
 *     handle's kernel -- SFL_STATE_LANE (one env per lane, sfl_counters.kernel_variant == 0, and the host build) or
 *     SFL_STATE_WAVE (every wave kernel) -- and a record is restored into a handle of the same class only.
 *   The bytes do not depend on block scheduling: two captures of an unchanged handle are identical.
 * sfl_state_info: the sizes, the layout class and the fingerprint of what a record depends on (the map descriptor,
 *   gamma, default_q, ntab, max_steps, delay_threshold, which malfunction stream is set, the layout class).
 * sfl_state_capture counts (device passes; the live bitmap and the offsets stay on the device) and returns the
 *   offsets, with which the caller sizes the buffers of sfl_state_read, which gathers, copies out (a NULL pointer
 *   skips one) and releases the device buffers.  A second sfl_state_capture replaces a pending one.
 * sfl_state_restore writes n records into n listed slots: each slot's Q block becomes default_q plus the record's
 *   rows, its key set and state arrays the record's, and the handle's host copy of the seeds follows.  No other env
 *   is touched.  The epsilon / lr schedule tables (sfl_hparams, sfl_set_hparam_groups) and a Flatland malfunction
 *   table (sfl_set_mf_schedule, indexed by slot) are the handle's, not the record's: the caller keeps them in step.
 *   Not state: sfl_counters.decisions and a running curve's cells.
 * sfl_state_ms: device time of the last capture (count + gather kernels) and of the last restore (0 on the host build).
 * Refused, with the handle unchanged (everything is checked on the host before the first device write): a
 *   graph-partitioned handle, one in external-action mode, an evaluation handle; an env or slot out of range or listed
 *   twice; sfl_state_read without a pending capture; a layout class or fingerprint other than the handle's; row_off /
 *   cell_off that do not start at 0, decrease, or do not end at n_rows / n_cells; a row id >= rows_per_env or not
 *   strictly ascending within an env; an env whose cell count is not the sum of its rows' widths. */
#define SFL_STATE_LANE 0u
#define SFL_STATE_WAVE 1u
typedef struct {
  uint64_t fingerprint;
  uint64_t q_per_env;
  uint32_t state_bytes;     /* bytes of one env's state record */
  uint32_t layout;          /* SFL_STATE_LANE or SFL_STATE_WAVE */
  uint32_t touched_words;
  uint32_t rows_per_env;
  uint32_t seed_offset;     /* byte offset of the env's seed (uint64) in its record */
  uint32_t pad_;
} sfl_state_desc;
int sfl_state_info(sfl_handle* h, sfl_state_desc* out);
int sfl_state_capture(sfl_handle* h, uint32_t n, const uint32_t* envs, uint64_t* row_off /* [n + 1] */,
                      uint64_t* cell_off /* [n + 1] */);
int sfl_state_read(sfl_handle* h, uint8_t* state /* [n][state_bytes] */, uint32_t* touched /* [n][touched_words] */,
                   uint32_t* row_ids /* [row_off[n]] */, uint64_t* cells /* [cell_off[n]] */);
int sfl_state_restore(sfl_handle* h, uint64_t fingerprint, uint32_t layout, uint32_t n, const uint32_t* slots,
                      const uint8_t* state, const uint32_t* touched, const uint64_t* row_off, const uint32_t* row_ids,
                      uint64_t n_rows, const uint64_t* cell_off, const uint64_t* cells, uint64_t n_cells);
int sfl_state_ms(sfl_handle* h, double* capture_ms, double* restore_ms /* either may be NULL */);
#ifdef __cplusplus
}
#endif
#endif /* SFL_H */
