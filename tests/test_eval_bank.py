"""Policy-bank evaluation on the host build (runtime.EvalBatch, sfl_bank_*; cases and references: tests/_evalbank.py):
the lane-per-env body's bank mode against the twin batch and the oracle, the fold against its numpy restatement, the
refusals, eval.py's --batch entry point, and the ABI."""
import configparser
import ctypes as C
import importlib
import json
import os
import pickle
import subprocess

import numpy as np
import pytest

from oracle import sfl_oracle as so
from tests import _evalbank as eb
from tests import _qfuzz as qf
from tests import _shapes as sh
from tests import hostsim

runtime = sh.runtime
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")
N = sh.n_envs(8)  # 35 envs


@pytest.mark.parametrize("S,T", [(16, 8), (16, 17), (16, 33), pytest.param(257, 64, marks=pytest.mark.slow)])
def test_twin_equality(S, T):
    """Cases 1 - 3: per-env outputs, at_dest, end state and table equal the twin's, for e % 3 and then its permutation
    on the same handle; the bank is unchanged afterwards."""
    eb.run_twin_equality(hostsim.lib(), eb.row(S, T), N, expect=(0, 1))


@pytest.mark.parametrize("S,T", [(16, 8), (16, 17), (16, 33), (5, 1)])
def test_long_episodes(S, T):
    """Table (a) alone, max_steps = 100,000: terminated episodes, unequal across the seeds of one policy; early, late and
    not arrived all occur over the three maps; a policy without episodes has NaN means."""
    t = eb.run_long(hostsim.lib(), eb.row(S, T), N if S != 5 else 19, classes=S != 5)
    if S == 5:  # some envs do not arrive
        assert (t.out["arrived"][0] == 0).any() and (t.out["arrived"][0] == 1).any()


def test_oracle_sampled_envs():
    """Three envs of (16, 8) against the oracle's test() with the table loaded as a dict."""
    rw = eb.row(16, 8)
    cm = sh.compiled(rw)
    pol = eb.assign(N, "mod")
    ev = eb.bank(hostsim.lib(), rw, N, qf.MAX_STEPS)
    try:
        got = ev.evaluate(pol)
        dicts = [ev.policy_dict(p) for p in range(eb.P)]
    finally:
        ev.close()
    for e in (0, 16, N - 1):
        _, model = so.build(sh.scenario(rw), qf.seeds(N)[e], sh.HP, max_steps=qf.MAX_STEPS, trace=False)
        model.q = {k: list(v) for k, v in dicts[pol[e]].items()}
        cum, arrived, delays = model.test()
        assert qf.same_bits(got["cum_reward"][e:e + 1], np.array([cum], np.float64)), e
        assert int(got["arrived"][e]) == arrived and got["delays"][:, e].astype(float).tolist() == [float(d) for d in delays], e
    assert cm.T == got["delays"].shape[0]


def test_policy_dict_round_trip():
    rw = eb.row(16, 8)
    ev = eb.bank(hostsim.lib(), rw, 4, qf.MAX_STEPS)
    try:
        for p in range(eb.P):
            d = ev.policy_dict(p)
            ev.load_policy_dict(p, d)
        assert not eb.bank_unchanged(ev, rw)
    finally:
        ev.close()


def test_truncation():
    eb.run_truncation(hostsim.lib(), eb.row(16, 8), N)


def test_epoch_wrap():
    eb.run_epoch_wrap(hostsim.lib(), 8)


def test_copy_policy():
    eb.run_copy_policy(hostsim.lib(), eb.row(16, 8))


def test_refusals():
    """Case 7: every entry point that needs a per-env table or a learner says "evaluation handle"; bad arguments raise
    with a message; after the refusals the handle still evaluates correctly."""
    lib = hostsim.lib()
    rw = eb.row(16, 8)
    cm = sh.compiled(rw)
    n = 9
    pol = eb.assign(n, "mod")
    ev = eb.bank(lib, rw, n, qf.MAX_STEPS)
    try:
        d, h = lib.dll, ev.h
        u64, u32, f64, i32 = (np.zeros(8 * n, t) for t in (np.uint64, np.uint32, np.float64, np.int32))
        q, tw = np.zeros(cm.q_per_env), np.zeros((cm.rows_per_env + 31) // 32, np.uint32)
        ra = _lib.RunArgs()
        ra.n_episodes, ra.stats_cap = 1, 0
        grp = (_lib.HParamGroup * 1)()
        u16 = np.zeros(n, np.uint16)
        own = np.zeros(cm.S, np.int32)
        p = runtime._ptr
        calls = dict(
            sfl_learn_begin=lambda: d.sfl_learn_begin(h, p(u64, C.c_uint64)),
            sfl_apply_qinit=lambda: d.sfl_apply_qinit(h, 1, p(u32, C.c_uint32), p(u32, C.c_uint32), p(f64, C.c_double)),
            sfl_learn=lambda: d.sfl_learn(h, C.byref(ra)),
            sfl_test=lambda: d.sfl_test(h, C.byref(ra)),
            sfl_step=lambda: d.sfl_step(h, 5, None, None),
            sfl_get_q=lambda: d.sfl_get_q(h, 0, p(q, C.c_double), p(tw, C.c_uint32)),
            sfl_set_q=lambda: d.sfl_set_q(h, 0, p(q, C.c_double), p(tw, C.c_uint32)),
            sfl_consensus=lambda: d.sfl_consensus(h, 0, 0, 1, None, None),
            sfl_curve_begin=lambda: d.sfl_curve_begin(h, 1, 1, 1, None, 4),
            sfl_part_config=lambda: d.sfl_part_config(h, 0, 1, p(own, C.c_int32), 0, n, n, 2 * n),
            sfl_env_begin=lambda: d.sfl_env_begin(h),
            sfl_env_begin_wave=lambda: d.sfl_env_begin_wave(h),
            sfl_set_hparam_groups=lambda: d.sfl_set_hparam_groups(h, 1, grp, p(u16, C.c_uint16)),
        )
        for name, call in calls.items():
            assert call() == -1, name
            msg = d.sfl_last_error().decode()
            assert "evaluation handle" in msg and msg.startswith(name + ": "), (name, msg)
        # arguments: a policy out of range, n_policies = 0, an unset policy
        eb.with_pytest_raises(lambda: ev.evaluate([eb.P] + list(pol[1:])), "policy 3 of 3")
        eb.with_pytest_raises(lambda: ev.set_policy_raw(eb.P, *eb.tables(rw)[0]), "policy 3 of 3")
        eb.with_pytest_raises(lambda: runtime.EvalBatch(cm, sh.HP, qf.seeds(n), 0, lib=lib), "n_policies")
        msg = eb.with_pytest_raises(lambda: runtime.EvalBatch(cm, sh.HP, qf.seeds(n), 1, lib=lib, delay_threshold=1 << 20),
                                    "delay_threshold out of range")  # (a refusal of the shared create path)
        assert "sfl_create_eval: delay_threshold" in msg and "sfl_create:" not in msg, msg
        with pytest.raises(ValueError):
            ev.copy_policy(0, ev)
        with pytest.raises(ValueError):
            ev.evaluate(pol[:-1])
        ev4 = runtime.EvalBatch(cm, sh.HP, qf.seeds(n), 4, lib=lib, max_steps=qf.MAX_STEPS)
        try:
            for i, tb in enumerate(eb.tables(rw)):
                ev4.set_policy_raw(i, *tb)
            eb.with_pytest_raises(lambda: ev4.evaluate([3] * n), "never set")
            eb.with_pytest_raises(lambda: ev4.copy_policy(3, ev, env=0), "evaluation handle")
            got = ev4.evaluate(pol)  # ... and the handle still evaluates
            assert got["table"]["episodes"].tolist() == [3, 3, 3, 0]
        finally:
            ev4.close()
        # what keeps working on an evaluation handle
        assert ev.kernel_note == "" or isinstance(ev.kernel_note, str)
        assert d.sfl_set_stream(h, None) == 0
        got = ev.evaluate(pol)
        assert not eb.mismatches(ev, got, eb.twin(rw, n, pol, qf.MAX_STEPS), pol)
        assert ev.counters()["last_launch_decisions"] == int(got["decisions"].sum())
        last, total = ev.fold_ms()
        assert last == 0.0 and total == 0.0  # (the host build)
    finally:
        ev.close()
    b = runtime.Batch(cm, sh.HP, [1], lib=lib, ntab=sh.NTAB)  # the bank calls on a training handle
    try:
        assert lib.dll.sfl_bank_eval(b.h, runtime._ptr(np.zeros(1, np.uint32), C.c_uint32), None) == -1
        assert "not an evaluation handle" in lib.dll.sfl_last_error().decode()
    finally:
        b.close()


def test_flatland_malfunction_schedule():
    """sfl_set_mf_schedule works as on a training handle: the bank run on Flatland's malfunction stream equals the twin's."""
    rw = eb.row(16, 8)
    cm, n = sh.compiled(rw), 5
    lib = hostsim.lib()
    tw = runtime.Batch(cm, sh.HP, qf.seeds(n), lib=lib, ntab=sh.NTAB, max_steps=qf.MAX_STEPS, malfunction_stream="flatland")
    ev = runtime.EvalBatch(cm, sh.HP, qf.seeds(n), 1, lib=lib, max_steps=qf.MAX_STEPS, malfunction_stream="flatland")
    try:
        for e in range(n):
            tw.set_q_raw(e, *eb.tables(rw)[0])
        ev.set_policy_raw(0, *eb.tables(rw)[0])
        ref, got = tw.test(1), ev.evaluate()
        for k in eb.OUT_KEYS:
            assert qf.same_bits(got[k], ref[k][0]), k
        assert not qf.same_bits(ref["num_malfunctions"][0], eb.twin(rw, N, eb.assign(N, "a"), qf.MAX_STEPS).out["num_malfunctions"][0][:n])
    finally:
        tw.close()
        ev.close()


# ---- case 9: the entry point ------------------------------------------------------------------------------------------------
def _experiment(tmp_path, name, sc_path, seed, table, default_q=0.0):
    """``sc_path``: a saved scenario file, or the name of a mapgen config (generated from ``seed``)."""
    exp = tmp_path / name
    exp.mkdir()
    cfg = configparser.ConfigParser()
    cfg["MISC"] = dict(random_seed=seed, out_dir=str(exp), checkpoint_freq=1000, exploit_freq=1000)
    cfg["ENV"] = dict(scenario=sc_path, malfunction_rate=0.01, min_duration=5, max_duration=15)
    cfg["MODEL"] = dict(num_episodes=1, gamma=1.0, epsilon=0.5, epsilon_decay_rate=0.9997, lr=0.1, lr_decay_rate=1.0,
                        default_q=default_q)
    with open(exp / "config.ini", "w") as f:
        cfg.write(f)
    with open(exp / "distr_q_model.pkl", "wb") as f:
        pickle.dump(table, f)
    return exp


def test_eval_entry_point(tmp_path, monkeypatch):
    evalmod = importlib.import_module("eval")
    lib = hostsim.lib()
    rw = eb.row(16, 8)
    cm = sh.compiled(rw)
    sc_path = str(tmp_path / "scenario.json")
    sh.scenario(rw).save(sc_path)
    hp = dict(gamma=1.0, epsilon=0.5, epsilon_decay_rate=0.9997, lr=0.1, lr_decay_rate=1.0, default_q=0.0)
    tabs = []
    for seed in (900, 901):  # two learners' tables (default_q 0, as the configs say)
        b = runtime.Batch(cm, hp, [seed], lib=lib, ntab=sh.NTAB)
        b.learn(20)
        tabs.append(b.q_dict(0))
        b.close()
    exps = [_experiment(tmp_path, f"exp{i}", sc_path, 450 + i, tabs[i]) for i in range(2)]
    made = []
    real = runtime.EvalBatch
    monkeypatch.setattr(runtime, "EvalBatch", lambda *a, **kw: made.append(1) or real(*a, **kw))
    n = 7
    res = evalmod.evaluate_batch([str(x) for x in exps], n, lib=lib)
    assert len(made) == 1 and sorted(res) == sorted(str(x) for x in exps)
    plain = evalmod.evaluate([str(x) for x in exps], lib=lib)
    ld = lambda d, f: np.load(os.path.join(d, f + ".npz"), allow_pickle=True)["x"]  # noqa: E731
    for i, exp in enumerate(exps):
        pe = np.load(exp / "eval_batch" / "per_env.npz", allow_pickle=True)
        assert pe["seeds"].tolist() == [450 + i + k for k in range(n)]
        assert float(ld(exp / "eval_0", "cum_reward")) == float(pe["cum_reward"][0]) == plain[str(exp)][0][0]
        assert ld(exp / "eval_0", "delays").tolist() == pe["delays"][0].tolist()
        assert ld(exp / "eval_0", "trains_at_dest").tolist() == pe["trains_at_dest"][0].tolist()
        with open(exp / "eval_batch" / "summary.json") as f:
            sm = json.load(f)
        out = dict(cum_reward=pe["cum_reward"], arrived=pe["arrived"], num_malfunctions=pe["num_malfunctions"],
                   decisions=pe["decisions"], ticks=pe["ticks"], delays=pe["delays"].T.astype(np.int32))
        cells = eb.restate(out, pe["at_dest"].T, pe["truncated"], [0] * n, 1, cm.T)
        assert {k: sm["cell"][k] for k in _lib.EVAL_FIELDS} == {k: int(cells[k][0]) for k in _lib.EVAL_FIELDS}
        assert sm["seeds"] == pe["seeds"].tolist() and sm["kernel_variant"] == 0 and sm["kernel_ms"] == 0.0
        assert sm["cell"]["early_mean"] == cells["trains_early"][0] / n
    assert len({tuple(np.load(x / "eval_batch" / "per_env.npz")["ticks"].tolist()) for x in exps}) == 2


def test_eval_entry_point_generated_maps(tmp_path, monkeypatch):
    """Two experiments that name the same mapgen config under different seeds are two maps and two timetables
    (main.build_scenario generates the config from random_seed): each gets an EvalBatch of its own, on its own map, and
    env 0 of each is the episode evaluate() runs.  A third experiment on the first one's seed shares its batch."""
    evalmod = importlib.import_module("eval")
    main = importlib.import_module("main")
    lib = hostsim.lib()
    hp = dict(gamma=1.0, epsilon=0.5, epsilon_decay_rate=0.9997, lr=0.1, lr_decay_rate=1.0, default_q=0.0)
    exps, cms = [], []
    for i, (seed, learn_seed) in enumerate(((450, 450), (451, 451), (450, 7))):
        cfg = configparser.ConfigParser()
        cfg["MISC"] = dict(random_seed=seed)
        cfg["ENV"] = dict(scenario="c1", malfunction_rate=0.01, min_duration=5, max_duration=15)
        cm = sh.comp.compile_scenario(main.build_scenario(cfg))
        b = runtime.Batch(cm, hp, [learn_seed], lib=lib, ntab=sh.NTAB)
        b.learn(20)
        exps.append(_experiment(tmp_path, f"gen{i}", "c1", seed, b.q_dict(0)))
        cms.append(cm)
        b.close()
    assert not np.array_equal(cms[0].arrays["tr_ed"], cms[1].arrays["tr_ed"]) or \
        not np.array_equal(cms[0].arrays["grid"], cms[1].arrays["grid"]), "precondition: the two seeds give two scenarios"
    made = []
    real = runtime.EvalBatch
    monkeypatch.setattr(runtime, "EvalBatch", lambda *a, **kw: made.append(kw.get("n_policies", a[3] if len(a) > 3 else None)) or real(*a, **kw))
    n = 5
    res = evalmod.evaluate_batch([str(x) for x in exps], n, lib=lib)
    assert sorted(made) == [1, 2] and len(res) == 3
    assert [res[str(x)]["n_policies"] for x in exps] == [2, 1, 2]
    plain = evalmod.evaluate([str(x) for x in exps], lib=lib)
    ld = lambda d, f: np.load(os.path.join(d, f + ".npz"), allow_pickle=True)["x"]  # noqa: E731
    for exp in exps:
        pe = np.load(exp / "eval_batch" / "per_env.npz", allow_pickle=True)
        assert float(pe["cum_reward"][0]) == float(ld(exp / "eval_0", "cum_reward")) == plain[str(exp)][0][0], exp
        assert int(pe["arrived"][0]) == plain[str(exp)][0][1], exp
        assert pe["delays"][0].tolist() == ld(exp / "eval_0", "delays").tolist(), exp
        assert pe["trains_at_dest"][0].tolist() == ld(exp / "eval_0", "trains_at_dest").tolist(), exp


# ---- case 10: the ABI -------------------------------------------------------------------------------------------------------
NEW = ("sfl_create_eval", "sfl_bank_set", "sfl_bank_get", "sfl_bank_copy", "sfl_bank_eval", "sfl_bank_read", "sfl_bank_fold_ms")


def test_abi():
    assert _lib.ABI_VERSION == 9 and hostsim.lib().dll.sfl_abi_version() == 9
    assert all(n in _lib.EXPORTS for n in NEW)
    header = open(os.path.join(os.path.dirname(build.HERE), "include", "sfl.h")).read()
    for n in NEW:
        assert f"int {n}(" in header, n
    libs = [hostsim.lib().path]
    if os.path.exists(build.PRODUCT_LIB):  # (the GPU file builds it and checks it there; here only if it is built)
        libs.append(build.PRODUCT_LIB)
    for path in libs:
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
        assert not [n for n in NEW if n not in exported], path
    assert len(_lib.EVAL_FIELDS) * 8 == 120
