"""Seed schedules on the MI355X: the device against the host build of the lane body, bit for bit -- Q-table, key set,
env state, the running episodes' seeds and the curve cells.  One cell per kernel family at ``_shapes.n_envs(G)`` envs
(more than one block, no multiple of the envs per block); each runs the truncating step schedule of
tests/_seedsched.py (max_steps 40; launches of 50, 130 and 130 decisions) with a pool of 3, held-out exploit rounds
and ``curve_exploit(2)``: the envs of a wavefront stand in different episodes, the pool wraps inside a launch, and
launches end inside episodes and inside exploit rounds.  The host references are computed once per cell
(``_seedsched.host_stepped``); tests/test_seed_schedule.py checks the host build against the oracle."""
import importlib

import numpy as np
import pytest

from tests import _golden, _seedsched as ss, _shapes as sh, hostsim

pytestmark = pytest.mark.gpu

runtime = sh.runtime
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")
aec = importlib.import_module("network-distributed-q-learning_amd.aec")
comp = importlib.import_module("network-distributed-q-learning_amd.compiler")

POOL, HELD = 3, True
# (row, SFL_WAVE_G or "scalar", hyperparameter groups): the kernel family each cell must run on
CELLS = (
    (ss.ROW_8, 8, False),        # k_wave_g, eight envs per wavefront
    (ss.ROW_17, 16, False),      # four envs per wavefront, a train in the second slot
    (ss.ROW_LM, 32, False),      # the row with the map tables in LDS
    (ss.ROW_32, 32, False),      # two envs per wavefront
    (ss.ROW_33, 64, False),      # k_wave
    (ss.ROW_65, 64, False),      # k_wave2
    (ss.ROW_17, "scalar", False),  # the lane-per-env body
    (ss.ROW_17, 16, True),       # the grouped instantiation
)


def _cid(c):
    return f"{c[0][0]}x{c[0][1]}k{c[0][2]}-g{c[1]}" + ("-hpg" if c[2] else "")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


def _select(monkeypatch, g):
    for k in ("SFL_KERNEL", "SFL_WAVE_G", "SFL_LDS_MAP", "SFL_REQUIRE_WAVE"):
        monkeypatch.delenv(k, raising=False)
    if g == "scalar":
        monkeypatch.setenv("SFL_KERNEL", "scalar")
    else:
        monkeypatch.setenv("SFL_WAVE_G", str(g))


def _predict(row, g, n):
    if g == "scalar":
        return 0, 1
    cm = sh.compiled(row)
    v = sh.choose_variant(cm.S, cm.T, n, sh.lm_bytes(cm.H, cm.W, cm.K), {"SFL_WAVE_G": str(g)})
    return v, sh.group_lanes(v)


def _equal(got, ref, what):
    bad = ss.mismatches(got, ref)
    assert not bad, f"{what}: {bad[:4]}"


def _same_curve(a, b):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(a[k]).dtype.kind == "f"), k


@pytest.mark.parametrize("cell", CELLS, ids=_cid)
def test_device_equals_host(lib, monkeypatch, cell):
    row, g, hpg = cell
    n = sh.n_envs(g if g != "scalar" else 32)
    refs = ss.host_checkpoints(row, n, POOL, HELD, hpg)
    ref_snap, ref_curve = refs[0]
    # preconditions, on the host twin: the schedule changed what was learned; the schedule's last launch ended inside
    # a held-out round, the two further ones inside episodes of pool index 2 and 0 (episodes truncated at max_steps
    # keep a batch's envs in lock step; external-action mode's cells below hold envs at different indices)
    plain_snap, _ = ss.host_stepped(row, n, None, False, hpg)
    assert ss.mismatches(ref_snap, plain_snap)
    sds_ref = sh.hpg_seeds(n) if hpg else sh.seeds(n)
    kinds = [{next((k for k in (0, 1, 2, ss.HELD_OUT) if ss.episode_seed(sd, k) == int(es)), None)
              for sd, es in zip(sds_ref, snap[1])} for snap, _ in refs]
    assert kinds == [{ss.HELD_OUT}, {2}, {0}], kinds
    _select(monkeypatch, g)
    kw = dict(hparam_groups=sh.GROUPS, env_group=sh.env_groups(n)) if hpg else {}
    sds = sh.hpg_seeds(n) if hpg else sh.seeds(n)
    b = ss.stepped(row, sds, lib, POOL, HELD, hp=sh.HANDLE_HP if hpg else ss.HP, **kw)
    try:
        c = b.counters()
        assert (c["kernel_variant"], c["group_lanes"]) == _predict(row, g, n), c
        if g == 32 and row == ss.ROW_LM:
            assert sh.VARIANTS[c["kernel_variant"]][4] == 1  # the LM row
        _equal(ss.snapshot(b), ref_snap, "host build")
        _same_curve(b.curve(), ref_curve)
        for d, (snap, curve) in zip(ss.MORE_CHUNKS, refs[1:]):
            b.step(d)
            _equal(ss.snapshot(b), snap, f"host build after step({d})")
            _same_curve(b.curve(), curve)
        assert b.seed_schedule() == (POOL, HELD)
    finally:
        b.close()


def _aec_run(cm, sds, lib, kernel, steps=90):
    b = aec.AECBatch(cm, sds, lib=lib, seed_pool=POOL, max_steps=25, kernel=kernel)
    out = b.step(None)
    rec = []
    for k in range(steps):
        acts = []
        for e in range(len(sds)):
            s = int(out["agent"][e])
            if s < 0:
                acts.append(-1)
            elif e % 3 == 1 and k % 17 == 16:
                acts.append(aec.ACTION_RESET)
            else:
                m = b.action_mask(e)
                acts.append(len(m) - 1 if k % 3 == 2 else int(np.flatnonzero(m)[0]))
        out = b.step(acts)
        rec.append({k_: np.array(v) for k_, v in out.items()})
        rec[-1]["episode_seeds"] = b.batch.episode_seeds()
    c = b.batch.counters()
    b.close()
    return rec, c


@pytest.mark.parametrize("kernel,g", (("lane", 16), ("wave", 16), ("wave", 64)))
def test_external_action_mode(lib, monkeypatch, kernel, g):
    cm = comp.compile_scenario(_golden.load("c2_mf")["scenario_obj"])
    n = sh.n_envs(g)
    sds = [11 + e for e in range(n)]
    want, _ = _aec_run(cm, sds, hostsim.lib(), "lane")
    # precondition, on the host twin: episodes ended, resets came mid-episode, the seeds moved off the base, and the
    # envs of one wavefront stand at different pool indices
    assert any((r["agent"] < 0).any() for r in want)
    assert (want[-1]["episode_seeds"] != np.array(sds, np.uint64)).any()
    first = [next(k for k in range(3) if ss.episode_seed(sd, k) == int(es))
             for sd, es in zip(sds[:4], want[-1]["episode_seeds"][:4])]
    assert len(set(first)) >= 2, first
    _select(monkeypatch, g)
    got, c = _aec_run(cm, sds, lib, kernel)
    assert (c["kernel_variant"] > 0) == (kernel == "wave") and (kernel == "lane" or c["group_lanes"] == g), c
    for k, (x, y) in enumerate(zip(got, want)):
        ended = y["agent"] < 0
        for f in y:
            if f in ("train", "slot", "state", "mask", "reward", "now"):  # (defined where an observation was emitted)
                assert np.array_equal(x[f][~ended], y[f][~ended]), (k, f)
            elif f in ("malfunctions", "truncated"):
                assert np.array_equal(x[f][ended], y[f][ended]), (k, f)
            elif f == "delays":
                assert np.array_equal(x[f][:, ended], y[f][:, ended]), (k, f)
            else:
                assert np.array_equal(x[f], y[f]), (k, f)


def test_capture_restore(lib, monkeypatch):
    row, g = ss.ROW_17, 16
    _select(monkeypatch, g)
    sds = sh.seeds(sh.n_envs(g))
    picked, slots = [1, 6, 18], [2, 0, 4]
    a = ss.stepped(row, sds, lib, POOL, HELD, chunks=(50, 130))
    st = a.capture(picked)
    small = ss.batch(row, [7, 8, 9, 10, 11], lib=lib, pool=POOL, heldout=HELD, max_steps=ss.TRUNC_STEPS)
    small.learn_begin()
    small.apply_qinit()
    small.restore(st, into=slots)
    small.curve_begin(2, 8, ring=131, exploit_freq=2)
    for b in (a, small):
        b.step(130)
    ref_snap, _ = ss.host_stepped(row, len(sds), POOL, HELD)
    ga, gs = ss.snapshot(a), ss.snapshot(small)
    _equal(ga, ref_snap, "host build")
    for e, s in zip(picked, slots):
        assert sh.same_env(gs[0][s], ga[0][e]) == [] and int(gs[1][s]) == int(ga[1][e]), (e, s)
    a.close()
    small.close()


def test_default_schedule_changes_nothing(lib, monkeypatch):
    row, g = ss.ROW_17, 16
    _select(monkeypatch, g)
    n = sh.n_envs(g)
    res = []
    for call in (False, True):
        b = ss.batch(row, sh.seeds(n), lib=lib, max_steps=ss.TRUNC_STEPS)
        if call:
            b.set_seed_schedule(1, False)
        b.learn_begin()
        b.apply_qinit()
        b.curve_begin(2, 8, ring=131, exploit_freq=2)
        for d in ss.TRUNC_CHUNKS:
            b.step(d)
        res.append((ss.snapshot(b), b.curve()))
        b.close()
    _equal(res[1][0], res[0][0], "the batch that never called the setter")
    _same_curve(res[1][1], res[0][1])
    ref_snap, ref_curve = ss.host_stepped(row, n, None, False)
    _equal(res[0][0], ref_snap, "host build")


def test_return_to_the_default_on_the_device(lib, monkeypatch):
    """A handle that has left the default and returned to pool 1 / flags 0 keeps launching the scheduled kernels, which
    run the rule: the episode in flight ends on its own seed, every later one on the base seed."""
    row, g = ss.ROW_17, 16
    n = sh.n_envs(g)

    def run(the_lib):
        b = ss.batch(row, sh.seeds(n), lib=the_lib, pool=0, max_steps=ss.TRUNC_STEPS)
        b.learn_begin()
        b.apply_qinit()
        b.step(100)
        mid = b.episode_seeds().copy()
        b.set_seed_schedule(1, False)
        b.step(7)
        kept = b.episode_seeds().copy()
        b.step(130)
        out = ss.snapshot(b), mid, kept
        b.close()
        return out

    ref, mid, kept = run(hostsim.lib())
    # on the host twin: the call came inside episodes off the base seed, which went on, and the base seed came back
    assert (mid != np.array(sh.seeds(n), np.uint64)).all() and (kept == mid).any()
    assert ref[1].tolist() == sh.seeds(n)
    _select(monkeypatch, g)
    got, gmid, gkept = run(lib)
    assert gmid.tolist() == mid.tolist() and gkept.tolist() == kept.tolist()
    _equal(got, ref, "host build")
