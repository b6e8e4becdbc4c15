"""The cases of tests/test_tick_sempass_gpu.py (the tick's one pass over the semaphore records: the records of the
trains that became done in the tick deleted, those of stopped and malfunctioning trains retimed) and what the host
build's run of each case went through, computed once per case and shared: per-episode statistics (a learning curve with
one env per series and one episode per bin) and every env's state at every launch boundary.  tests/test_tick_sempass.py
checks on the host build alone that no case is vacuous."""
import dataclasses
import functools
import importlib
from collections import namedtuple

import numpy as np

from tests import hostsim

mapgen = importlib.import_module("network-distributed-q-learning_amd.mapgen")
comp = importlib.import_module("network-distributed-q-learning_amd.compiler")
runtime = importlib.import_module("network-distributed-q-learning_amd.runtime")
parity = importlib.import_module("network-distributed-q-learning_amd.parity")

MALFUNCTION = (0.2, 2, 6)  # stopped and malfunctioning trains on most ticks
HP = dict(gamma=1.0, epsilon=0.5, epsilon_decay_rate=0.9997, lr=0.1, lr_decay_rate=1.0, default_q=0.0)
NTAB = 1 << 14
E = 64
SEEDS = [7100 + i for i in range(E)]
N_BINS = 128  # more than the episodes any env ends: every cell of the curve is one episode


def _schedule(long_launches, ones):
    """One-decision launches (a launch boundary after every decision, so also between an arrival's tick and the next
    one) between launches of a few hundred decisions."""
    out = []
    for n in long_launches:
        out += [1] * ones + [n]
    return tuple(out + [1] * ones)


# cfg, SFL_WAVE_G, group lanes of the kernel, decisions per launch, max_episode_steps (None: the map's own)
Case = namedtuple("Case", "cfg G lanes schedule mes", defaults=(None,))
C3 = _schedule((500, 800, 900, 900, 900), 10)
C2 = _schedule((150, 200, 100), 25)
CASES = (
    Case("c3", 16, 16, C3),     # variant 7, the bench's kernel (which a batch of 64 envs gets with SFL_WAVE_G=16)
    Case("c3", 64, 64, C3),
    Case("c2", 8, 8, C2),
    Case("c2", 16, 16, C2),
    Case("c2", 32, 32, C2),
    Case("c2", 16, 16, C2, 30),  # every episode ends at max_episode_steps with trains still on the map
)


def case_id(c):
    return f"{c.cfg}-g{c.G}" + (f"-mes{c.mes}" if c.mes else "")


@functools.lru_cache(maxsize=None)
def compiled(cfg, mes=None):
    sc = mapgen.make_config(cfg, malfunction=MALFUNCTION)
    if mes is not None:
        sc = dataclasses.replace(sc, max_episode_steps=mes)
    return comp.compile_scenario(sc)


Ref = namedtuple("Ref", "episodes arrived ended_by_steps arrival_then_tick_across_a_launch")


@functools.lru_cache(maxsize=None)
def reference(cfg, schedule, mes):
    """What the host build's run of the case went through (the same for every group size)."""
    cm = compiled(cfg, mes)
    b = runtime.Batch(cm, HP, SEEDS, lib=hostsim.lib(), ntab=NTAB)
    try:
        b.learn_begin()
        b.apply_qinit()
        b.curve_begin(1, N_BINS, series=list(range(E)), ring=max(schedule) + 1)
        across = 0
        prev = None
        for n in schedule:
            b.step(n)
            ep = b.curve()["episodes"].copy()
            st = [parity.env_state(b, e) for e in range(E)]
            if prev is not None and n == 1:
                for e in range(E):
                    (el0, _, _, _, bits0), (el1, _, _, _, bits1) = prev[1][e], st[e]
                    done0, done1 = (bits0 >> 21) & 1, (bits1 >> 21) & 1
                    # a train done at the last boundary, and this launch ticked on in the same episode
                    if prev[0][e] == ep[e] and el1 > el0 and (done0 & done1).any() and not done1.all():
                        across += 1
            prev = (ep, st)
        c = b.curve()
        assert int(c["lost"].sum()) == 0 and int(c["count"].max()) == 1
        one = c["count"] == 1
        # (the curve's own `truncated` is the decision limit max_steps, never reached here: an episode that ended
        # with trains still on the map ended at max_episode_steps)
        assert int(c["truncated"].sum()) == 0
        return Ref(c["episodes"].copy(), np.where(one, c["arrived_sum"], -1), int((one & (c["all_arrived"] == 0)).sum()), across)
    finally:
        b.close()


def ref_of(c):
    return reference(c.cfg, c.schedule, c.mes)


def check_reference(c):
    """The reference alone went through what the case is for."""
    r, T = ref_of(c), compiled(c.cfg, c.mes).T
    assert int(r.episodes.min()) >= 2, "every env ends at least two episodes"
    assert r.arrival_then_tick_across_a_launch >= 1, "an arrival, a launch boundary, then further ticks of the episode"
    assert int(((r.arrived >= 1) & (r.arrived < T)).sum()) >= 1, "an episode with some trains arrived and some not"
    assert r.ended_by_steps >= 1, "an episode ended at max_episode_steps with trains still on the map"
