"""The cases of tests/test_phase_scalars_gpu.py (decide() and post() read the map's and the state's learner scalars as
one block at their top: sfl_core.h MapDecide / MapLearn / MapUpdate / StateLearn) and the host build's run of each,
computed once per case and shared.  tests/test_phase_scalars.py checks on the host build and the oracle that no case is
vacuous.

What can go wrong is a field read at the wrong place of the reordered structs, a path that reads a field its block does
not carry, or a value that changed between two launches and is read stale.  So beside the shapes (every group size, the
bench's kernel, the largest map) the conditions move every field of the blocks off the value the benchmark gives it:

  base      the benchmark's hyperparameters (gamma 1, default_q 0, no lr decay)
  gamma     gamma 0.9 and default_q 0.5
  lr_in     a decaying lr inside its table (post() takes the table path and reads the interaction count)
  lr_past   a decaying lr and a table of 48 entries: the run stops with the lr-table error.  (The host build has no
            such flag -- sfl_core.h raises it in device code only, where the pow is not the host's -- so the host side of
            this case is that its counts pass the table's end, and the device side that the error comes)
  short     a table of 48 entries without lr decay: crossed inside a launch, epsilon from the pow past it
  notable   SFL_SEEDSEQ_TABLE=0: MapDecide::seedseq32 is null
  flatland  malfunction_stream="flatland": the per-env malfunction table set after create
  delay0    delay_threshold = 0
  exploit   exploit_freq = 1 and episodes cut after 38 decisions: greedy rounds between learning launches
  targets   learn(2), step(57), learn(3), step(1): the episode target and the decision budget change from launch to
            launch (episodes cut after 61 decisions)
  resume    suspend in the middle of the schedule, resume into a fresh handle, step on

Every run is 63 envs (four blocks at G = 16, the last one short of an env) over tests/_decide_loads.py's schedules:
one-decision launches between launches of a few hundred decisions."""
import functools
import importlib
from collections import namedtuple

import numpy as np

from oracle import sfl_oracle as so
from tests import _decide_loads as D
from tests import _sempass as S
from tests import _shapes as sh
from tests import hostsim

runtime = D.runtime
parity = D.parity

E = 63
SEEDS = D.SEEDS[:E]
NTAB = S.NTAB
SHORT_NTAB = 48
HP = S.HP
LR_DECAY = dict(HP, lr_decay_rate=0.9995)
SCHEDULES = D.SCHEDULES


def resume_at(cfg):
    """The launch in front of which the batch is suspended: among the one-decision launches between the first two long
    ones, so that launches of one and of hundreds lie on both sides."""
    return [i for i, k in enumerate(SCHEDULES[cfg]) if k > 1][1] - 2


TARGET_MAX_STEPS = 60
LEARN_KEYS = ("cum_reward", "arrived", "num_malfunctions", "delays", "decisions", "ticks")

# cond -> (hyperparameters, Batch keyword arguments, environment)
CONDS = dict(
    base=(HP, {}, {}),
    gamma=(dict(HP, gamma=0.9, default_q=0.5), {}, {}),
    lr_in=(LR_DECAY, {}, {}),
    lr_past=(LR_DECAY, dict(ntab=SHORT_NTAB), {}),
    short=(HP, dict(ntab=SHORT_NTAB), {}),
    notable=(HP, {}, {"SFL_SEEDSEQ_TABLE": "0"}),
    flatland=(HP, dict(malfunction_stream="flatland"), {}),
    delay0=(HP, dict(delay_threshold=0), {}),
    exploit=(HP, dict(max_steps=D.EXPLOIT_MAX_STEPS), {}),
    targets=(HP, dict(max_steps=TARGET_MAX_STEPS), {}),
    resume=(HP, {}, {}),
)
# what parity.check_batch can drive itself: learn_begin, the optimistic init, the schedule
PLAIN = ("base", "gamma", "lr_in", "short", "notable", "flatland", "delay0")
# two groups that differ in epsilon and in the lr schedule, one of them decaying
GROUPS = (dict(HP, epsilon=0.9, epsilon_decay_rate=0.999), dict(HP, epsilon=0.1, lr=0.3, lr_decay_rate=0.9995))

Case = namedtuple("Case", "cfg G cond")
SHAPES = (Case("c2", 8, "base"), Case("c2", 16, "base"), Case("c2", 32, "base"), Case("c3", 16, "base"),
          Case("c3", 64, "base"))
CONDITIONS = tuple(Case(cfg, 16, cond) for cond in CONDS if cond != "base" for cfg in ("c3", "c2"))
BIG = (255, 128, 8, 4242)  # variant 5's trains full, tests/_shapes.py


def case_id(c):
    return f"{c.cfg}-g{c.G}-{c.cond}"


def hp_of(cond):
    return CONDS[cond][0]


def kwargs(cond):
    return dict(dict(ntab=NTAB), **CONDS[cond][1])


def env_vars(c):
    return dict(SFL_WAVE_G=str(c.G), **CONDS[c.cond][2])


def make(cfg, cond, lib):
    return runtime.Batch(D.compiled(cfg), hp_of(cond), SEEDS, lib=lib, **kwargs(cond))


Run = namedtuple("Run", "outs final streams")


def drive(b, cfg, cond, fresh=None, streams=False):
    """Drive a batch through the case; ``fresh()``: a new handle for the resume case (the old one is closed).  Returns
    the batch that finished and (what every launch returned, the final snapshot, the stream words per launch)."""
    sch, outs, words = SCHEDULES[cfg], [], []
    if cond == "targets":
        outs = [b.learn(2), b.step(57)[0], b.learn(3), b.step(1)[0]]
        return b, Run(outs, D.snapshot(b), words)
    b.learn_begin()
    b.apply_qinit()
    if cond == "exploit":
        b.curve_begin(1, 4, ring=max(sch) + 2, exploit_freq=D.EXPLOIT_FREQ)
    if streams:
        words.append(D.stream_words(b))
    for i, k in enumerate(sch):
        if cond == "resume" and i == resume_at(cfg):
            state = b.capture()
            b.close()
            b = fresh()
            b.learn_begin()
            b.apply_qinit()
            b.restore(state)
        outs.append(b.step(k)[0])
        if streams:
            words.append(D.stream_words(b))
    return b, Run(outs, D.snapshot(b), words)


@functools.lru_cache(maxsize=None)
def reference(cfg, cond):
    """The host build's run of the case (the same for every group size).  The resume case's reference is the run that
    never stops."""
    if cond == "resume":
        return reference(cfg, "base")
    b = make(cfg, cond, hostsim.lib())
    try:
        b, r = drive(b, cfg, cond, streams=cond == "exploit")
        return r
    finally:
        b.close()


def outs_differ(got, ref):
    """The launches whose results differ: decision counts, or a learn()'s per-episode arrays."""
    bad = []
    for i, (g, r) in enumerate(zip(got, ref)):
        if isinstance(r, dict):
            bad += [f"launch {i}: {k}" for k in LEARN_KEYS if not np.array_equal(g[k], r[k])]
        elif g != r:
            bad.append(f"launch {i}: {g} decisions, the host build {r}")
    return bad + (["number of launches"] if len(got) != len(ref) else [])


def envs_that_differ(a, b):
    """The envs whose Q-table or state differs between two final snapshots."""
    return [e for e, (x, y) in enumerate(zip(a, b))
            if not np.array_equal(x[0], y[0]) or parity._state_diff(x[2], y[2])]


@functools.lru_cache(maxsize=None)
def table_crossings(cfg, cond, n_envs=8):
    """Of the first n_envs envs of a short-table case on the oracle, those in which some switch's interaction count
    stands below the table's length before one of the long launches and at or past it behind it."""
    sc, out = D.compiled(cfg).scenario, []
    for e in range(n_envs):
        env, model = so.build(sc, SEEDS[e], hp_of(cond), trace=False)
        st, crossed = None, False
        for k in SCHEDULES[cfg]:
            before = dict(st["counts"]) if st else {}
            st = so.run_decisions(model, k, st) if st else so.run_decisions(model, k)
            crossed |= k > 1 and any(before.get(a, 0) < SHORT_NTAB <= n for a, n in st["counts"].items())
        if crossed:
            out.append(e)
    return out


def greedy_between_learning(cfg):
    """The envs of the exploit case with a one-decision launch inside a greedy round (the stream stood) that has
    launches which moved the stream -- learning decisions -- before it and behind it."""
    r, sch, out = reference(cfg, "exploit"), SCHEDULES[cfg], []
    for e in range(E):
        moved = [not np.array_equal(r.streams[i][e], r.streams[i + 1][e]) for i in range(len(sch))]
        if any(sch[j] == 1 and not moved[j] and any(moved[:j]) and any(moved[j + 1:]) for j in range(len(sch))):
            out.append(e)
    return out


# ---- the largest map, G = 64 (tests/_shapes.py's row, hyperparameters and chunks) ---------------------------------------
def big_envs():
    return sh.n_envs(64)


# ---- the policy bank on two banks in turn (tests/_evalbank.py) -----------------------------------------------------------
def rotated(policy, by=1):
    from tests import _evalbank as EB
    return tuple((p + by) % EB.P for p in policy)
