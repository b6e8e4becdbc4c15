"""The wave kernels' numeric envelope: the scenarios, cases and cached references of tests/test_field_limits.py (CPU)
and tests/test_field_limits_gpu.py.  tests/_shapes.py pins every kernel shape on its size limits; these pin the three
places where the device code differs from the host build of the lane body and which no other test executes:

A. the 8-bit (switch, train) slot epoch (sfl_core.h slot_make): on reset 256, and every 255 resets after it, every
   slot word of the env is cleared -- serially in env_reset, lane-strided over the wave kernels' [E][T][S] layout in
   sfl_wave.h reset(), from eblk[EB_EPOCH] in the partitioned step;
B. the wave kernels' 32-bit semaphore record (sfl_wave.h r_pack: t0 14 bits signed, t1 - t0 9 bits) on and one past
   the limits choose_variant admits: t_hi = 8191 and span <= 511;
C. the exploratory draw's Lemire rejection (the ``slow`` branch of sfl_wave.h's egreedy), which needs three allowed
   actions and a sub-generator whose first 32-bit output is 0, and the same branch taken by a device that holds no
   2^31-entry table (SFL_SEEDSEQ_TABLE=0).

Out of scope: the int16 distance staging (dist < 32767) needs a path of 32,766 cells, which mapgen cannot build; the
lower side of the 14-bit start tick (ed_min - 2 >= -8192) needs negative departures, which Flatland timetables do not
have."""
import copy
import functools
from collections import namedtuple

import numpy as np

from oracle import sfl_oracle as so
from tests import _shapes as sh
from tests import hostsim

runtime, parity, mapgen = sh.runtime, sh.parity, sh.mapgen

# ---- sfl_core.h / sfl_engine.h restated (tests/test_field_limits.py reads them from the headers) ------------------
EPOCH_BITS = 8
R_T0_BITS, R_DUR_BITS = 14, 9
T_HI_MAX = (1 << (R_T0_BITS - 1)) - 1  # 8191
SPAN_MAX = (1 << R_DUR_BITS) - 1       # 511
NOTE_HORIZON = "timetable horizon beyond 8191 ticks"
NOTE_SPAN = "a semaphore span beyond 511 ticks"


def row_of(S, T, K=8):
    row = [r for r in sh.ROWS if r[:3] == (S, T, K)]
    assert len(row) == 1, (S, T, K)
    return row[0]


def span_and_t_hi(cm, sc):
    """choose_variant's span and t_hi (sfl_engine.h) of a compiled scenario."""
    dist_max = max(0, int(np.max(cm.arrays["tr_init_dist"])))
    len_max = max(0, int(np.max(cm.arrays["port_len"])))
    span = max(dist_max, 2 * len_max + 2) + 4
    ed_max = max(0, max(t.earliest_departure for t in sc.trains))
    return span, max(ed_max, sc.max_episode_steps) + 2 + span


def sem_fields(sem):
    """(present, t0, t1) of 64-bit semaphore records (sfl_core.h sem_pack: t0 16 | t1 16 | owner 8 | in 1 | present 1)."""
    sem = np.asarray(sem, np.uint64)
    t0 = (sem & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16).astype(np.int32)
    t1 = ((sem >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16).astype(np.int32)
    return ((sem >> np.uint64(41)) & np.uint64(1)).astype(bool), t0, t1


# ---- A. the epoch wrap --------------------------------------------------------------------------------------------
# Every episode is cut after max_steps + 1 = 8 decisions.  learn(600, exploit_freq=50) resets 612 times (the 12 exploit
# episodes reset too), the step path's 4,244 decisions 531 times: both pass the clears of resets 256 and 511.  The
# first chunk ends 4 decisions into the episode that reset 256 begins (255 * 8 = 2,040 decisions precede it).
EPOCH_MAX_STEPS = 7
EPOCH_LEARN = dict(n_episodes=600, exploit_freq=50)
EPOCH_CHUNKS = (2044, 2200)
EPOCH_RESETS = 520  # at least this many, counted on the oracle
WRAPS = (1 << EPOCH_BITS, 2 * (1 << EPOCH_BITS) - 1)  # the resets that clear: 256 and 511

Case = namedtuple("Case", "row G kernel")  # kernel: the SFL_KERNEL setting, if any

# one per kernel family: (row, group size): grouped with one train slot per lane (G = 8, 16, 32, and variant 11 with the
# map in LDS), with two (G = 16), k_wave, k_wave2, and the lane-per-env kernel
EPOCH_CASES = (Case(row_of(16, 8), 8, None), Case(row_of(16, 16), 16, None), Case(row_of(16, 17), 16, None),
               Case(row_of(16, 32), 32, None), Case(row_of(16, 16, 3), 32, None), Case(row_of(64, 32), 64, None),
               Case(row_of(64, 65), 64, None), Case(row_of(16, 17), 16, "scalar"))
EPOCH_HPG = Case(row_of(16, 16), 16, None)
EPOCH_PART = Case(row_of(64, 33), 64, None)
EPOCH_ROWS = tuple(dict.fromkeys(c.row for c in EPOCH_CASES + (EPOCH_HPG, EPOCH_PART)))


def case_id(c):
    S, T, K = c.row[:3]
    return f"{S}x{T}k{K}-g{c.G}" + (f"-{c.kernel}" if c.kernel else "")


def case_env(c):
    env = {"SFL_WAVE_G": str(c.G)}
    if c.kernel:
        env["SFL_KERNEL"] = c.kernel
    return env


def predict(c, key=None):
    """(kernel_variant, group_lanes) the engine must report for a case (``key``: the scenario, if not the row's)."""
    cm = sh.compiled(key or c.row)
    v = sh.choose_variant(cm.S, cm.T, sh.n_envs(c.G), sh.lm_bytes(cm.H, cm.W, cm.K), case_env(c))
    return v, sh.group_lanes(v)


def epoch_host_learn(row, n):
    return sh.host_learn(row, EPOCH_MAX_STEPS, n, **EPOCH_LEARN)


def epoch_oracle_learn(row, seed):
    return sh.oracle_learn(row, seed, EPOCH_MAX_STEPS, False, **EPOCH_LEARN)


def epoch_learn_mismatches(out, e, ref):
    return sh.learn_mismatches(out, e, ref, **EPOCH_LEARN)


def epoch_host_plain(row, n):
    return sh.host_plain(row, EPOCH_CHUNKS, n, EPOCH_MAX_STEPS)


@functools.lru_cache(maxsize=None)
def oracle_stepped(row, seed, total, max_steps=100_000, group=None):
    """The oracle's run_decisions: (Q dict, the number of decisions made before each reset)."""
    env, model = so.build(sh.scenario(row), seed, sh.HP if group is None else sh.GROUPS[group], max_steps=max_steps,
                          trace=False)
    state = dict(rng=np.random.default_rng(model.seed), counts={a: 0 for a in env.agents}, t=0, in_episode=False,
                 pending={}, at_dest=[], it=None, done=0)
    at, inner = [], env.reset

    def reset(*a, **kw):
        at.append(state["done"])
        return inner(*a, **kw)

    env.reset = reset
    so.run_decisions(model, total, state)
    return model.q, at


def epoch_oracle_plain(row, seed, group=None):
    return oracle_stepped(row, seed, sum(EPOCH_CHUNKS), EPOCH_MAX_STEPS, group)


# ---- B. the semaphore record's limits -------------------------------------------------------------------------------
# An episode runs all of its ~8,160 ticks (the late trains never arrive): 16,000 - 33,000 decisions per env.  The
# 9-train row learns two full episodes (the exploit round at t = 0, then the learn one); the 33-train row one, which
# already costs the oracle ~10 s.  HORIZON_CHUNKS: sfl_step chunks after the second of which the host build's envs
# (some of them, on the 33-train row) stand past tick 8000 of their first episode.
HORIZON_LEARN = {(16, 9): dict(n_episodes=1, exploit_freq=1), (64, 33): dict(n_episodes=1, exploit_freq=None)}
HORIZON_CHUNKS = {(16, 9): (15000, 1200), (64, 33): (15000, 1400)}
LATE = 61  # the last of the late trains departs this many ticks before the episode's end


def _horizon(row, over):
    """The row's scenario with max_episode_steps rewritten so that choose_variant's t_hi is 8191 + over, and every
    third train's timetable moved to the last ~100 ticks of the episode."""
    base = sh.scenario(row)
    span, _ = span_and_t_hi(sh.compiled(row), base)
    sc = copy.deepcopy(base)
    sc.max_episode_steps = T_HI_MAX - 2 - span + over
    late = sc.trains[::3]
    shift = sc.max_episode_steps - LATE - max(t.earliest_departure for t in late)
    for t in late:
        t.earliest_departure += shift
        t.latest_arrival += shift
    sc.name = "horizon"
    return sc


def horizon_key(row, over=0):
    key = ("horizon",) + tuple(row) + (over,)
    sh.DERIVED.setdefault(key, functools.partial(_horizon, row, over))
    return key


def span_key(spacing):
    """generate(5, 3, 2, seed=4242, spacing=): at 126 len_max = 251 and span 508, at 127 253 and 512.  Every generated
    map has a segment through a corner of the line grid, 2 spacing - 1 cells, so spans are 4 spacing + 4: 508 is the
    nearest under 511 that the generator reaches."""
    key = ("span", spacing)
    sh.DERIVED.setdefault(key, lambda: mapgen.generate(5, 3, 2, seed=4242, spacing=spacing, malfunction=(0.01, 5, 15),
                                                       name="span"))
    return key


HORIZON_CASES = (Case(row_of(16, 9), 16, None), Case(row_of(16, 9), 32, None), Case(row_of(64, 33), 64, None))
SPAN_ON, SPAN_PAST = 126, 127
SPAN_GS = (8, 64)
SPAN_CHUNKS = (100, 200)  # ~30 episodes of ~10 decisions; the oracle takes ~1 s per 100 decisions of this map


def durations(b, n):
    """The largest t1 - t0 and the largest t0 over the present semaphore records of a batch's first n envs."""
    dur = t0m = -1
    for e in range(n):
        p, t0, t1 = sem_fields(parity.env_state(b, e)[2])
        if p.any():
            dur, t0m = max(dur, int((t1 - t0)[p].max())), max(t0m, int(t0[p].max()))
    return dur, t0m


@functools.lru_cache(maxsize=None)
def host_stepped_snapshots(key, chunks, n, max_steps=100_000):
    """The host build stepped through ``chunks``: the snapshot after each chunk and (largest duration, largest t0)
    over the present semaphores at each."""
    b = runtime.Batch(sh.compiled(key), sh.HP, sh.seeds(n), lib=hostsim.lib(), ntab=sh.NTAB, max_steps=max_steps)
    b.learn_begin()
    b.apply_qinit()
    snaps, seen = [], []
    for k in chunks:
        assert b.step(k)[0] == k * n
        snaps.append(sh.snapshot(b, n))
        seen.append(durations(b, n))
    b.close()
    return snaps, seen


# ---- C. the rejected exploratory draw -------------------------------------------------------------------------------
# The only sub-seeds in [0, 2^31 - 1) whose generator's first 32-bit output is 0 (scripts/lemire_rejects.cpp scans them
# all); with three allowed actions Lemire rejects that draw and numpy's integers(0, 3) gives 2.
REJECTING = (838496653, 448450445)
# controls: the table's ends, byte offset 4 GiB into it, and k_seedseq_table's grid-stride seam (16,384 x 256 threads)
CONTROLS = ((1 << 31) - 2, 1 << 30, 4194303, 4194304, 0, 1)
SUB_SEEDS = REJECTING + CONTROLS
SUB_RANGE = (1 << 31) - 1  # rng.integers(0, np.iinfo(np.int32).max)
HP_EXPLORE = dict(sh.HP, epsilon=1.0, epsilon_decay_rate=1.0)
GROUPS_EXPLORE = (HP_EXPLORE, dict(HP_EXPLORE, lr=0.4))
DRAW_STEPS = 20
# (row, group size): the rows whose first decision has three allowed actions
DRAW_CASES = ((row_of(5, 1), 16), (row_of(5, 1), 32), (row_of(5, 1), 64), (row_of(16, 8), 8), (row_of(16, 33), 16),
              (row_of(16, 33), 64), (row_of(65, 32), 64), (row_of(128, 64), 64))
DRAW_CASES = tuple(Case(r, g, None) for r, g in DRAW_CASES)
DRAW_HPG = Case(row_of(16, 33), 64, None)
DRAW_PART = Case(row_of(65, 32), 64, None)
DRAW_ROWS = tuple(dict.fromkeys(c.row for c in DRAW_CASES))


def crafted_buffer(v):
    """The buffered 32-bit word from which numpy's integers(0, 2^31 - 1) returns v without rejecting: the smallest u
    with (u * (2^31 - 1)) >> 32 == v whose low product word is at least (2^32 mod (2^31 - 1)) = 2."""
    u = -(-(v << 32) // SUB_RANGE)
    while (u * SUB_RANGE) & 0xFFFFFFFF < 2:
        u += 1
    assert (u * SUB_RANGE) >> 32 == v and u < 1 << 32
    return u


def crafted_state(seed, v):
    """default_rng(seed)'s five state words (runtime.numpy_rng_state) with has_uint32 = 1 and uinteger = the crafted
    buffer: random() does not touch the buffer, so the first exploring decision's sub-seed is v."""
    st = runtime.numpy_rng_state(seed)
    st[4] = (1 << 32) | crafted_buffer(v)
    return st


def numpy_generator(words):
    """A numpy Generator in the state of five such words."""
    g = np.random.default_rng(0)
    st = g.bit_generator.state
    st["state"] = dict(state=(int(words[0]) << 64) | int(words[1]), inc=(int(words[2]) << 64) | int(words[3]))
    st["has_uint32"], st["uinteger"] = int(words[4]) >> 32, int(words[4]) & 0xFFFFFFFF
    g.bit_generator.state = st
    return g


def draw_sub_seeds(n):
    return [SUB_SEEDS[e % len(SUB_SEEDS)] for e in range(n)]


def draw_states(seeds, subs=None):
    subs = draw_sub_seeds(len(seeds)) if subs is None else subs
    return np.array([crafted_state(s, v) for s, v in zip(seeds, subs)], dtype=np.uint64)


def learn_begin_with(b, states):
    """sfl_learn_begin with raw generator states, one row of five words per env."""
    import ctypes as C
    states = np.ascontiguousarray(states, np.uint64)
    assert states.shape == (b.E, 5)
    b.lib.check(b.lib.dll.sfl_learn_begin(b.h, states.ctypes.data_as(C.POINTER(C.c_uint64))), "sfl_learn_begin")


def draw_run(b, states, steps=DRAW_STEPS):
    learn_begin_with(b, states)
    b.apply_qinit()
    assert b.step(steps)[0] == steps * b.E


@functools.lru_cache(maxsize=None)
def host_draw(row, n, grouped=False):
    """The host build given the crafted states, after step(20): the snapshot of every env."""
    kw = dict(hparam_groups=GROUPS_EXPLORE, env_group=sh.env_groups(n)) if grouped else {}
    b = runtime.Batch(sh.compiled(row), sh.HANDLE_HP if grouped else HP_EXPLORE, sh.seeds(n), lib=hostsim.lib(),
                      ntab=sh.NTAB, **kw)
    draw_run(b, draw_states(sh.seeds(n)))
    ref = sh.snapshot(b, n)
    b.close()
    return ref


@functools.lru_cache(maxsize=None)
def oracle_draw(row, seed, v, group=None):
    """The oracle's run_decisions(20) from the crafted state: its Q dict, and the action mask and action of the first
    decision."""
    env, model = so.build(sh.scenario(row), seed, HP_EXPLORE if group is None else GROUPS_EXPLORE[group], trace=False)
    state = dict(rng=numpy_generator(crafted_state(seed, v)), counts={a: 0 for a in env.agents}, t=0, in_episode=False,
                 pending={}, at_dest=[], it=None, done=0)
    first, inner = [], env.last

    def last():
        r = inner()
        if not first:
            first.append(np.array(r[4]["action_mask"]).copy())
        return r

    def on_step(env_, obs, action, r, post):
        if len(first) == 1:
            first.append(int(action))

    env.last, model.on_step = last, on_step
    so.run_decisions(model, DRAW_STEPS, state)
    return dict(q=model.q, mask=first[0], action=first[1])


# the plain sweep cases (tests/_shapes.py CASES) run again on a device without the table: one per kernel family
NO_TABLE_CASES = tuple(c for c in sh.CASES if c.mode == "plain" and (c.row[:3], c.G) in (
    ((16, 8, 8), 8), ((16, 17, 8), 16), ((16, 16, 3), 32), ((64, 32, 8), 64), ((129, 64, 8), 64)))
NO_TABLE_DRAW = tuple(c for c in DRAW_CASES if (c.row[:2], c.G) in (((16, 8), 8), ((16, 33), 64)))
