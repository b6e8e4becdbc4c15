"""The recording's entry points on the host build (cases 9 and 11 of tests/test_record.py's list):
DistrQLearning.test(plot=True), ASyncSwitchEnv.render() and eval.py --batch N --record K [--diagnose] [--frames]."""
import importlib
import os

import numpy as np
import pytest

from tests import _evalbank as eb
from tests import _qfuzz as qf
from tests import _record as rc
from tests import _shapes as sh
from tests import hostsim
from tests.test_eval_diag import _experiment

runtime = sh.runtime
parity = sh.parity
env_mod = importlib.import_module("network-distributed-q-learning_amd.env")
distr_q = importlib.import_module("network-distributed-q-learning_amd.distr_q")
render = importlib.import_module("network-distributed-q-learning_amd.render")
HP = dict(gamma=1.0, epsilon=0.5, epsilon_decay_rate=0.9997, lr=0.1, lr_decay_rate=1.0, default_q=0.0)
PX = 8


def test_distr_q_test_plot(tmp_path):
    """test(plot=True) of a one-env learner that has learned writes exactly `decisions` PNGs beside the three .npz
    files, and they load back with the frame's shape; plot=False writes the three .npz files and nothing else; a batch
    of two is refused with a pointer to EvalBatch.record."""
    from PIL import Image
    rw = eb.row(16, 8)
    cm = sh.compiled(rw)
    env = env_mod.ASyncSwitchEnv(sh.scenario(rw), max_steps=100_000)
    model = distr_q.DistrQLearning(env, seed=900, lib=hostsim.lib(), **HP)
    try:
        model.learn(5, str(tmp_path), checkpoint_freq=0)
        for f in os.listdir(tmp_path):
            os.remove(tmp_path / f)
        plain, plot = tmp_path / "plain", tmp_path / "plot"
        plain.mkdir()
        plot.mkdir()
        a = model.test(str(plain), plot=False)
        assert sorted(os.listdir(plain)) == ["cum_reward.npz", "delays.npz", "trains_at_dest.npz"]
        b = model.test(str(plot), plot=True)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
        n = int(model.batch.test(1)["decisions"][0][0])
        assert n > 10
        assert sorted(os.listdir(plot)) == sorted(["cum_reward.npz", "delays.npz", "trains_at_dest.npz"] +
                                                  [f"iter_{i}.png" for i in range(n)])
        for i in (0, n // 2, n - 1):
            assert np.asarray(Image.open(plot / f"iter_{i}.png").convert("RGB")).shape == (cm.H * PX, cm.W * PX, 3)
        for k in ("cum_reward.npz", "delays.npz", "trains_at_dest.npz"):
            assert np.array_equal(np.load(plain / k, allow_pickle=True)["x"], np.load(plot / k, allow_pickle=True)["x"])
    finally:
        model.batch.close()
    env2 = env_mod.ASyncSwitchEnv(sh.scenario(rw), max_steps=100_000, n_envs=2)
    two = distr_q.DistrQLearning(env2, seed=900, lib=hostsim.lib(), **HP)
    try:
        with pytest.raises(NotImplementedError, match="EvalBatch.record"):
            two.test(str(tmp_path), plot=True)
    finally:
        two.batch.close()


def test_env_render():
    """render() after a reset and three steps shows each on-map train of sfl_get_env_state at its cell; None with
    render_mode=None."""
    rw = eb.row(16, 32)
    cm = sh.compiled(rw)
    for mode in ("rgb_array", "human", None):
        env = env_mod.ASyncSwitchEnv(sh.scenario(rw), max_steps=100_000, render_mode=mode)
        try:
            env.reset(seed=300, lib=hostsim.lib())
            for _ in range(3):
                agent = next(env.agent_iter())
                mask = env.last()[4]["action_mask"]
                env.step(int(np.nonzero(mask)[0][0]))
            img = env.render()
            if mode is None:
                assert img is None
                continue
            pos = parity.env_state(env._aec.batch, 0)[3]
            on = np.nonzero(np.asarray(pos) >= 0)[0]
            assert len(on) > 0, "precondition: a train on the map"
            assert img.dtype == np.uint8 and img.shape == (cm.H * PX, cm.W * PX, 3)
            for h in on:
                r, c = divmod(int(pos[h]), cm.W)
                assert tuple(img[r * PX + PX // 2, c * PX + PX // 2]) == render.train_colour(h), h
            assert np.array_equal(img, env.render())
        finally:
            env.close()


def test_eval_entry_point_record(tmp_path):
    """eval.py --batch N --record 2 --diagnose writes the episode files of the first two jammed envs of each experiment
    (the batch has at least two), each equal to EvalBatch.recording's, traffic.npz and, with --frames, one PNG per
    recorded decision; without --record the files are those of today."""
    evalmod = importlib.import_module("eval")
    lib = hostsim.lib()
    rw = eb.row(16, 17)
    cm = sh.compiled(rw)
    sc_path = str(tmp_path / "scenario.json")
    sh.scenario(rw).save(sc_path)
    tabs = []
    for seed in (900, 901):
        b = runtime.Batch(cm, HP, [seed], lib=lib, ntab=sh.NTAB)
        b.learn(20)
        tabs.append(b.q_dict(0))
        b.close()
    n, stall, K = 6, 7, 2
    exps = [_experiment(tmp_path / "rec", f"exp{i}", sc_path, 450 + i, tabs[i]) for i in range(2)]
    evalmod.evaluate_batch([str(x) for x in exps], n, lib=lib, diagnose=True, stall=stall, record=K, frames=True)
    plain = [_experiment(tmp_path / "plain", f"exp{i}", sc_path, 450 + i, tabs[i]) for i in range(2)]
    evalmod.evaluate_batch([str(x) for x in plain], n, lib=lib, diagnose=True, stall=stall)
    # the same batch by hand
    seeds = [450 + i + k for i in range(2) for k in range(n)]
    pol = [p for p in range(2) for _ in range(n)]
    ev = runtime.EvalBatch(cm, HP, seeds, 2, lib=lib)
    try:
        for p in range(2):
            ev.load_policy_dict(p, tabs[p])
        ev.evaluate(pol)
        cls = ev.diagnose(stall=stall)["cls"]
        jammed = [[e for e in range(p * n, (p + 1) * n) if (cls[:, e] >= 4).any()] for p in range(2)]
        assert all(len(j) >= K for j in jammed), "precondition: two jammed envs per experiment"
        flat = [e for j in jammed for e in j[:K]]
        ev.record(flat)
        ev.evaluate(pol)
        want = {seeds[e]: ev.recording(k) for k, e in enumerate(flat)}
        traffic = [ev.traffic(p) for p in range(2)]
    finally:
        ev.close()
    for p, (exp, pl) in enumerate(zip(exps, plain)):
        d = exp / "eval_batch"
        mine = [seeds[e] for e in jammed[p][:K]]
        assert sorted(os.listdir(d)) == sorted(["nonarrivals.json", "per_env.npz", "summary.json", "traffic.npz"] +
                                               [f"episode_{s}.npz" for s in mine] + [f"frames_{s}" for s in mine])
        assert sorted(os.listdir(pl / "eval_batch")) == ["nonarrivals.json", "per_env.npz", "summary.json"]
        for k in ("nonarrivals.json", "summary.json"):
            assert open(d / k).read().replace(str(exp), "") == open(pl / "eval_batch" / k).read().replace(str(pl), "")
        pa, pb = (np.load(x / "eval_batch" / "per_env.npz", allow_pickle=True) for x in (exp, pl))
        assert sorted(pa.files) == sorted(pb.files)
        for k in pa.files:
            assert pa[k].dtype == pb[k].dtype and pa[k].shape == pb[k].shape, k
            assert all(np.array_equal(x, y) for x, y in zip(pa[k], pb[k])) if pa[k].dtype == object else qf.same_bits(pa[k], pb[k]), k
        for s in mine:
            ep = runtime.Episode.load(d / f"episode_{s}.npz")
            assert not rc.episode_mismatches(ep, want[s]) and ep.complete
            assert sorted(os.listdir(d / f"frames_{s}")) == sorted(f"iter_{i}.png" for i in range(ep.rows))
        z = np.load(d / "traffic.npz")
        assert z["seeds"].tolist() == mine
        for k in rc._lib.TRAFFIC_FIELDS:
            assert np.array_equal(z[k], traffic[p][k]), k
