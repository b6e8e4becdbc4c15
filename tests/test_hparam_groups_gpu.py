"""Hyperparameter groups on the MI355X: every kernel shape reads its env's group's epsilon / lr schedule -- grouped
HIP batches against the grouped host build, against ungrouped HIP batches per group, and against the oracle."""
import importlib

import numpy as np
import pytest

from oracle import sfl_oracle as so
from tests import hostsim

pytestmark = pytest.mark.gpu

mapgen = importlib.import_module("network-distributed-q-learning_amd.mapgen")
comp = importlib.import_module("network-distributed-q-learning_amd.compiler")
runtime = importlib.import_module("network-distributed-q-learning_amd.runtime")
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")

HP = dict(gamma=1.0, epsilon=0.5, epsilon_decay_rate=0.9997, lr=0.1, lr_decay_rate=1.0, default_q=0.0)
GRID = [dict(HP), dict(HP, epsilon=0.1), dict(HP, epsilon_decay_rate=0.99), dict(HP, lr=0.4),
        dict(HP, lr_decay_rate=0.999), dict(HP, epsilon=0.0), dict(HP, epsilon=1.0, epsilon_decay_rate=1.0)]
HANDLE_HP = dict(HP, epsilon=0.3, epsilon_decay_rate=0.95, lr=0.25, lr_decay_rate=0.99)  # matches no group
NTAB = 1 << 14


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


@pytest.fixture(params=["wave", "wave32", "wave8", "scalar", "wave64"])
def kernel(request, monkeypatch):
    """Which device kernel a Batch created inside the test runs (as tests/test_gpu.py's fixture: 'wave' = four envs
    per wavefront, 'wave32' two, 'wave8' eight, 'scalar' = k_run), plus 'wave64': one env per wavefront, the shapes
    that read the group's tables with scalar loads."""
    monkeypatch.delenv("SFL_KERNEL", raising=False)
    monkeypatch.delenv("SFL_WAVE_G", raising=False)
    if request.param == "scalar":
        monkeypatch.setenv("SFL_KERNEL", "scalar")
    else:
        monkeypatch.setenv("SFL_WAVE_G", {"wave": "16", "wave32": "32", "wave8": "8", "wave64": "64"}[request.param])
    return request.param


def _check_kernel(b, kernel, lanes=None):
    c = b.counters()
    assert (c["kernel_variant"] > 0) == (kernel != "scalar"), c
    if lanes is not None:
        assert c["group_lanes"] == lanes, c


def _stepped(cm, hp, seeds, lib, chunks, ntab=NTAB, **kw):
    b = runtime.Batch(cm, hp, seeds, lib=lib, ntab=ntab, **kw)
    b.learn_begin()
    b.apply_qinit()
    for n in chunks:
        got, _ = b.step(n)
        assert got == n * len(seeds)
    return b


def _same(a, ea, b, eb, what):
    qa, ta = a.q_raw(ea)
    qb, tb = b.q_raw(eb)
    assert np.array_equal(qa, qb) and np.array_equal(ta, tb), what


def _grid_parity(lib, kernel, cfg, grid, n_seeds, chunks, oracle_groups, lanes=None):
    """E = len(grid) * n_seeds envs, env e in group e % len(grid) (so one wavefront holds envs of different groups):
    every env equal to the grouped host build and to the ungrouped HIP batch of its group; some to the oracle."""
    sc = mapgen.make_config(cfg)
    cm = comp.compile_scenario(sc)
    G = len(grid)
    seeds0 = [1000 + i for i in range(n_seeds)]
    env_group = [e % G for e in range(G * n_seeds)]
    seeds = [seeds0[e // G] for e in range(G * n_seeds)]
    bg = _stepped(cm, HANDLE_HP, seeds, lib, chunks, hparam_groups=grid, env_group=env_group)
    _check_kernel(bg, kernel, lanes)
    bh = _stepped(cm, HANDLE_HP, seeds, hostsim.lib(), chunks, hparam_groups=grid, env_group=env_group)
    for e in range(len(seeds)):
        _same(bg, e, bh, e, f"env {e} vs the host build")
    firsts = []
    for g, hp in enumerate(grid):
        bu = _stepped(cm, hp, seeds0, lib, chunks)
        _check_kernel(bu, kernel, lanes)
        for i in range(n_seeds):
            _same(bg, g + G * i, bu, i, f"group {g} seed {seeds0[i]} vs ungrouped HIP")
        firsts.append(bu.q_raw(0)[0])
        bu.close()
    for a in range(G):  # the groups' tables differ pairwise: the parity cannot pass vacuously
        for b in range(a + 1, G):
            assert not np.array_equal(firsts[a], firsts[b]), (a, b)
    for g in oracle_groups:
        e = g + G * (g % n_seeds)
        _, model = so.build(sc, seeds[e], grid[g], trace=False)
        so.run_decisions(model, sum(chunks))
        assert bg.q_dict(e) == model.q, f"group {g} vs the oracle"
    bg.close()
    bh.close()


def test_c2_grid(lib, kernel):
    """c2, E = 35 (no multiple of any envs-per-block), 7 groups interleaved."""
    lanes = {"wave": 16, "wave32": 32, "wave8": 8, "wave64": 64, "scalar": 1}[kernel]
    _grid_parity(lib, kernel, "c2", GRID, 5, [37, 91, 250], range(len(GRID)), lanes)


@pytest.mark.parametrize("shape", ["wave", "wave32"])
def test_c3_grid(lib, monkeypatch, shape):
    """c3, E = 28: 'wave' is variant 7, the kernel built in its own translation unit."""
    monkeypatch.delenv("SFL_KERNEL", raising=False)
    monkeypatch.setenv("SFL_WAVE_G", "16" if shape == "wave" else "32")
    cm = comp.compile_scenario(mapgen.make_config("c3"))
    probe = runtime.Batch(cm, HP, [1], lib=lib, ntab=64)
    assert probe.counters()["kernel_variant"] == (7 if shape == "wave" else 9)
    probe.close()
    _grid_parity(lib, shape, "c3", GRID, 4, [150], (1, 4))


def test_c5_grid(lib, monkeypatch):
    """c5, E = 8 (4 groups x 2 seeds): one env per wavefront, two train slots per lane, scalar loads."""
    monkeypatch.delenv("SFL_KERNEL", raising=False)
    monkeypatch.delenv("SFL_WAVE_G", raising=False)
    # (groups whose schedules differ from the first decision on: in 100 decisions over 256 switches a switch's
    # interaction count stays near 0, where the two epsilon decay rates of GRID still agree)
    _grid_parity(lib, "wave", "c5", [GRID[0], GRID[1], GRID[3], GRID[4]], 2, [100], (), 64)


PAST = [dict(HP, epsilon=0.3, epsilon_decay_rate=0.99), dict(HP, epsilon=0.6, epsilon_decay_rate=0.999, lr=0.3),
        dict(HP, epsilon=0.2, epsilon_decay_rate=0.995, lr=0.05)]


def test_past_the_table(lib, kernel):
    """ntab = 64 and far more decisions per switch: epsilon past the table is the group's eps0 * pow(decay, n) and
    lr the group's lr0 (lr_decay 1.0 in every group).  Against ungrouped HIP only: the device pow is not libm's."""
    sc = mapgen.make_config("c2")
    cm = comp.compile_scenario(sc)
    seeds0 = [77, 78, 79]
    G = len(PAST)
    env_group = [e % G for e in range(G * len(seeds0))]
    seeds = [seeds0[e // G] for e in range(len(env_group))]
    bg = _stepped(cm, HANDLE_HP, seeds, lib, [900], ntab=64, hparam_groups=PAST, env_group=env_group)
    _check_kernel(bg, kernel)
    firsts = []
    for g, hp in enumerate(PAST):
        bu = _stepped(cm, hp, seeds0, lib, [900], ntab=64)
        for i in range(len(seeds0)):
            _same(bg, g + G * i, bu, i, f"group {g} seed {seeds0[i]}")
        firsts.append(bu.q_raw(0)[0])
        bu.close()
    assert not any(np.array_equal(firsts[a], firsts[b]) for a in range(G) for b in range(a + 1, G))
    _, model = so.build(sc, seeds0[0], PAST[0], trace=False)
    assert max(so.run_decisions(model, 900)["counts"].values()) > 64  # the pow path ran
    bg.close()


def test_decayed_lr_group_past_the_table_fails_loudly(lib, kernel):
    """The lr-table rule is per group: one group with a decaying lr past the table stops the launch, as an ungrouped
    handle with that lr_decay does; the same batch without that group runs."""
    cm = comp.compile_scenario(mapgen.make_config("c2"))
    bad = dict(HP, lr_decay_rate=0.999)
    seeds = [77, 78, 79, 80]
    b = runtime.Batch(cm, HP, seeds, lib=lib, ntab=64, hparam_groups=PAST + [bad], env_group=[0, 1, 2, 3])
    _check_kernel(b, kernel)
    b.learn_begin()
    b.apply_qinit()
    with pytest.raises(_lib.SflError, match="ntab"):
        b.step(900)
    b.close()
    u = runtime.Batch(cm, bad, seeds[:1], lib=lib, ntab=64)
    u.learn_begin()
    u.apply_qinit()
    with pytest.raises(_lib.SflError, match="ntab"):
        u.step(900)
    u.close()
    # (the handle's own lr_decay, 0.999, is no group's: it does not count)
    ok = _stepped(cm, bad, seeds[:3], lib, [900], ntab=64, hparam_groups=PAST, env_group=[0, 1, 2])
    ok.close()
