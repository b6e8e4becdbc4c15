"""External-action mode on the wave kernels (AECBatch(kernel="wave"), sfl_env_begin_wave): the (row, group size) cases
of the GPU sweep (tests/test_aec_wave_gpu.py), the run every case makes, and that run on the host build -- the
lane-per-env body env_run_ext, the reference every EXT kernel must equal bit for bit -- computed once per case and
shared.  tests/test_aec_wave.py checks the cases' coverage of the ten EXT cells and that no reference is vacuous."""
import functools
import importlib
from collections import namedtuple

import numpy as np

from tests import _shapes, hostsim
from tests.test_aec_device import fixed_policy

aec = importlib.import_module("network-distributed-q-learning_amd.aec")
parity = importlib.import_module("network-distributed-q-learning_amd.parity")

MAX_STEPS = 25      # every env truncates several times in CALLS calls
CALLS = 150
RESET_AT = 17       # one env with a pending observation gets ACTION_RESET at this call ...
WITHHOLD_AT = 23    # ... and one gets no action (-1) at this one
OUTPUTS = aec.AECBatch.FIELDS + ("arrived", "delays")

Case = namedtuple("Case", "row G max_steps calls", defaults=(MAX_STEPS, CALLS))


def _c(S, T, G, K=8, **kw):
    row = [r for r in _shapes.ROWS if r[:3] == (S, T, K)]
    assert len(row) == 1, (S, T, K)
    return Case(row[0], G, **kw)


# One case per EXT cell (variants 1 - 10), each on a row that fills the shape's trains (T == TW) or switches; then the
# rows one train or one switch past a shape's limit and k_wave2's rows with the second train slot in use and with every
# train / switch register in use; then a handle created on the LDS-map shape (variant 11), which steps variant 8.
SWEEP = (
    _c(16, 32, 64),      # 1: k_wave, T == TW, S at its limit
    _c(64, 32, 64),      # 2
    _c(64, 64, 64),      # 3
    _c(128, 64, 64),     # 4
    _c(64, 65, 64),      # 5: k_wave2, one train in the second slot
    _c(16, 16, 16),      # 6: G = 16, one train slot per lane, every lane a train
    _c(64, 32, 16),      # 7: G = 16, two slots per lane, full
    _c(16, 32, 32),      # 8: G = 32 (K = 8: the map tables do not fit variant 11)
    _c(64, 32, 32),      # 9
    _c(16, 8, 8),        # 10: G = 8, full
    _c(16, 17, 16),      # 7: the first train in the second slot
    _c(17, 8, 8),        # one switch past variant 10: no G = 8 shape fits, the handle is on variant 2 (G = 64)
    _c(5, 1, 8),         # 10: one train, lanes almost all idle
    _c(255, 128, 64),    # 5: every train slot
    _c(256, 127, 64),    # 5: every switch register
    _c(16, 32, 32, K=3),  # created on variant 11 (LM): steps its twin, variant 8
)
# reset 256 wraps the (switch, train) epoch: the wave reset()'s lane-strided slot clear.  max_steps = 3 ends an episode
# every four applied actions (five calls); one shape per kernel family
WRAP = (
    _c(16, 8, 8, max_steps=3, calls=1300),
    _c(16, 17, 16, max_steps=3, calls=1300),
    _c(16, 32, 64, max_steps=3, calls=1300),
    _c(129, 9, 64, max_steps=3, calls=1300),
)


def case_id(c):
    S, T, K, _ = c.row
    return f"{S}x{T}k{K}-g{c.G}" + ("" if c.max_steps == MAX_STEPS else f"-ms{c.max_steps}")


def predict(c):
    """(kernel_variant, group_lanes) a wave handle of the case reports: the created shape, the LM row as its twin."""
    v, g = _shapes.predict(_shapes.Case(c.row, c.G, "plain"))
    return (8, g) if v == 11 else (v, g)


def run(c, lib, kernel, cm=None, seeds=None, **kw):
    """The case's run on ``lib``: a copy of every output after every call, the launch counters of every call, every
    env's final state, the kernel the handle reports, and what the two special calls met."""
    cm = cm or _shapes.compiled(c.row)
    seeds = seeds or _shapes.seeds(_shapes.n_envs(c.G))
    b = aec.AECBatch(cm, seeds, lib=lib, max_steps=c.max_steps, kernel=kernel, **kw)
    try:
        return drive(b, cm, c.calls)
    finally:
        b.close()


def drive(b, cm, calls):
    outs, launches, special = [], [], {}
    out = b.step(None)
    for k in range(calls + 1):
        outs.append({key: out[key].copy() for key in OUTPUTS})
        cn = b.batch.counters()
        launches.append((cn["last_launch_decisions"], cn["last_launch_ticks"]))
        if k == calls:
            break
        acts = fixed_policy(cm, out["agent"], out["mask"], k)
        live = np.flatnonzero(out["agent"] >= 0)
        if k == RESET_AT and len(live):
            acts[int(live[0])] = aec.ACTION_RESET
            special["reset"] = int(live[0])
        if k == WITHHOLD_AT and len(live):
            acts[int(live[-1])] = -1
            special["withheld"] = int(live[-1])
        out = b.step(acts)
    cn = b.batch.counters()
    return dict(outs=outs, launches=launches, special=special, kernel=(cn["kernel_variant"], cn["group_lanes"]),
                states=[parity.env_state(b.batch, e) for e in range(b.E)])


@functools.lru_cache(maxsize=None)
def host_run(c):
    return run(c, hostsim.lib(), "lane")


def mismatches(got, ref):
    """Where two runs differ: (call, output) pairs, launch counters, env states (empty: bit-equal)."""
    bad = []
    for k, (a, b) in enumerate(zip(got["outs"], ref["outs"])):
        bad += [(k, key) for key in OUTPUTS if not np.array_equal(a[key], b[key])]
        if got["launches"][k] != ref["launches"][k]:
            bad.append((k, "launch counters", got["launches"][k], ref["launches"][k]))
        if len(bad) > 8:
            break
    for e, (x, y) in enumerate(zip(got["states"], ref["states"])):
        bad += [(f"env {e}", d) for d in parity._state_diff(x, y)]
    assert len(got["outs"]) == len(ref["outs"]) and got["special"] == ref["special"]
    return bad


def episode_ends(r):
    return sum(int((o["agent"] < 0).sum()) for o in r["outs"])
