// Stand-alone sanitizer check of the host side of sfl_env_step_dev / sfl_env_sync (scripts/aec_dev_asan.py builds
// and runs it with -fsanitize=address,undefined): the host build's sources with a main() of their own.  Reads a
// compiled map (the file aec_dev_asan.py writes: the sfl_map_desc scalars, its arrays in declaration order, the
// expected first observation row), makes a few device-call steps on two envs with the first allowed action, a
// host call in between, and checks env 0's first dense observation row.
#include <stdio.h>

#include <vector>

#include "../../network-distributed-q-learning_amd/csrc/sfl_hostsim.cpp"

static std::vector<char> blob(FILE* f) {
  uint64_t n = 0;
  if (fread(&n, 8, 1, f) != 1) exit(2);
  std::vector<char> b(n);
  if (n && fread(b.data(), 1, n, f) != n) exit(2);
  return b;
}

#define CHECK(call)                                            \
  if ((call) != 0) {                                           \
    fprintf(stderr, "%s: %s\n", #call, sfl_last_error());      \
    return 1;                                                  \
  }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  sfl_map_desc md{};
  int32_t sc[10];
  double rate;
  uint64_t qpe;
  if (fread(sc, 4, 10, f) != 10 || fread(&rate, 8, 1, f) != 1 || fread(&qpe, 8, 1, f) != 1) return 2;
  md.H = sc[0], md.W = sc[1], md.S = sc[2], md.T = sc[3], md.K = sc[4], md.max_episode_steps = sc[5];
  md.mf_min = sc[6], md.mf_max = sc[7], md.rows_per_env = (uint32_t)sc[8], md.delay_threshold = sc[9];
  md.mf_rate = rate;
  md.q_per_env = qpe;
  std::vector<std::vector<char>> a;
  for (int i = 0; i < 28; ++i) a.push_back(blob(f));
  int i = 0;
#define ARR(field, type) md.field = (const type*)a[i++].data();
  ARR(grid, uint16_t) ARR(cell_sw, int16_t) ARR(sw_np, uint8_t) ARR(sw_na, uint8_t) ARR(act_src, uint8_t)
  ARR(act_dst, uint8_t) ARR(act_turn, uint8_t) ARR(act_j, uint8_t) ARR(first_other, uint8_t) ARR(port_side, uint8_t)
  ARR(slot_nroutes, uint8_t) ARR(slot_route_act, uint8_t) ARR(q_w, uint8_t) ARR(port_nb, int16_t)
  ARR(port_len, int16_t) ARR(port_unique, int16_t) ARR(q_off, uint64_t) ARR(row_base, uint32_t) ARR(dist, int32_t)
  ARR(tr_ed, int32_t) ARR(tr_la, int32_t) ARR(tr_k, int32_t) ARR(tr_target, int32_t) ARR(tr_init_cell, int32_t)
  ARR(tr_init_dist, int32_t) ARR(tr_init_delay, int32_t) ARR(tr_init_dir, uint8_t) ARR(tr_init_port, int16_t)
  std::vector<char> want = blob(f);
  fclose(f);
  if (want.size() != SFL_OBS_WIDTH * 4) return 2;

  double tab[16];
  for (double& x : tab) x = 0.0;
  sfl_hparams hp{};
  hp.gamma = 1.0, hp.epsilon_decay_rate = 1.0, hp.lr_decay_rate = 1.0, hp.max_steps = 100000, hp.ntab = 16;
  hp.eps_tab = hp.lr_tab = tab;
  const uint32_t E = 2;
  const uint64_t seeds[E] = {450565, 7};
  sfl_handle* h = nullptr;
  CHECK(sfl_create(&md, &hp, E, seeds, 0, &h));
  CHECK(sfl_env_begin(h));
  const size_t T = md.T;
  std::vector<int32_t> act(E, -1), agent(E), train(E), slot(E), reward(E), now(E), nsw(E), snow(E), nmf(E), trunc(E),
      delays(T * E), nact(E);
  std::vector<uint32_t> state(E), mask(E), arrived(4 * E);
  alignas(16) int32_t obs[E * SFL_OBS_WIDTH];
  alignas(16) uint8_t amask[E * SFL_MAX_ACTIONS];
  std::vector<uint8_t> done(E);
  sfl_env_dev_io io{};
  io.io.agent = agent.data(), io.io.train = train.data(), io.io.slot = slot.data(), io.io.state = state.data();
  io.io.mask = mask.data(), io.io.reward = reward.data(), io.io.now = now.data(), io.io.next_switch = nsw.data();
  io.io.step_now = snow.data(), io.io.arrived = arrived.data(), io.io.malfunctions = nmf.data();
  io.io.delays = delays.data(), io.io.truncated = trunc.data();
  io.obs = obs, io.action_mask = amask, io.n_actions = nact.data(), io.done = done.data();
  CHECK(sfl_env_step_dev(h, &io));  // (null actions: the first observations)
  CHECK(sfl_env_sync(h));
  if (memcmp(obs, want.data(), want.size()) != 0) {
    fprintf(stderr, "env 0's first observation row differs\n");
    return 1;
  }
  io.io.actions = act.data();
  int applied = 0;
  for (int k = 0; k < 40; ++k) {
    for (uint32_t e = 0; e < E; ++e) {
      act[e] = -1;
      for (int j = 0; j < nact[e] && act[e] < 0; ++j)
        if (amask[e * SFL_MAX_ACTIONS + j]) act[e] = j;
    }
    if (k == 20) {  // a host call in between: the pending observations, as the device call left them
      sfl_env_io hio = io.io;
      hio.actions = nullptr;
      std::vector<int32_t> ag2(E);
      hio.agent = ag2.data();
      CHECK(sfl_env_step(h, &hio));
      for (uint32_t e = 0; e < E; ++e)
        if (agent[e] >= 0 && ag2[e] != agent[e]) return 1;
    }
    CHECK(sfl_env_step_dev(h, &io));
    for (uint32_t e = 0; e < E; ++e) applied += snow[e] >= 0;
  }
  CHECK(sfl_env_sync(h));
  CHECK(sfl_destroy(h));
  printf("aec_dev_asan ok: %d actions applied\n", applied);
  return applied > 0 ? 0 : 1;
}
