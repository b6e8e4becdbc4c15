"""decide() and post() read the learner's scalars of the map and the state as one block each at their top, and the
structs are reordered for it, on the MI355X.  Nothing may change a result: every env of every case equals the host
build -- Q-table, key set, env state, what every launch returned -- over schedules that put one-decision launches
between launches of a few hundred decisions.  tests/_phase_scalars.py has the cases (every field of the blocks moved
off the benchmark's value, values that change between launches); tests/test_phase_scalars.py asserts that none is
vacuous.  The kernels that keep their order (G = 64, external-action mode, the partitioned local step) and the
policy bank run on the reordered structs too, each against its host or fused twin."""
import importlib

import numpy as np
import pytest

from tests import _aec_wave as W, _decide_loads as D, _evalbank as EB, _phase_scalars as PS, _qfuzz as qf, _shapes as sh
from tests import hostsim
from tests import test_shape_edges_gpu as edges

pytestmark = pytest.mark.gpu

runtime = importlib.import_module("network-distributed-q-learning_amd.runtime")
parity = importlib.import_module("network-distributed-q-learning_amd.parity")
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")

SWITCHES = ("SFL_KERNEL", "SFL_WAVE_G", "SFL_LDS_MAP", "SFL_REQUIRE_WAVE", "SFL_ENV_KERNEL", "SFL_SEEDSEQ_TABLE")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _kernel(b, c):
    cn = b.counters()
    assert cn["kernel_variant"] > 0 and cn["group_lanes"] == c.G, cn
    if c.cfg == "c3" and c.G == 16:
        assert cn["kernel_variant"] == 7, cn  # the bench's kernel


@pytest.mark.parametrize("c", PS.SHAPES + PS.CONDITIONS, ids=PS.case_id)
def test_every_env_equals_the_host_build(lib, monkeypatch, c):
    for k, v in PS.env_vars(c).items():
        monkeypatch.setenv(k, v)
    b = PS.make(c.cfg, c.cond, lib)
    try:
        _kernel(b, c)
        if c.cond == "lr_past":
            # the host's counts pass the table's end inside a launch (tests/test_phase_scalars.py): the device stops
            # there instead of computing a pow that is not the host's
            with pytest.raises(_lib.SflError, match="ntab"):
                PS.drive(b, c.cfg, c.cond)
            return
        ref = PS.reference(c.cfg, c.cond)
        b, got = PS.drive(b, c.cfg, c.cond, fresh=lambda: PS.make(c.cfg, c.cond, lib))
        _kernel(b, c)  # (the resumed handle runs the same kernel)
        assert PS.outs_differ(got.outs, ref.outs) == []
        assert D.mismatches(got.final, ref.final) == []
        if c.cond in PS.PLAIN:
            assert parity.check_batch(b, PS.hp_of(c.cond), range(PS.E), PS.SCHEDULES[c.cfg], hostsim.lib(),
                                      **PS.kwargs(c.cond)) == []
    finally:
        b.close()


def test_two_groups_that_differ_in_epsilon_and_lr(lib, monkeypatch):
    """One batch, two hyperparameter groups (one with a decaying lr): the HPG kernels read the groups' rows and the
    map's ntab from the reordered structs."""
    monkeypatch.setenv("SFL_WAVE_G", "16")
    kw = dict(ntab=PS.NTAB, hparam_groups=PS.GROUPS, env_group=[e % 2 for e in range(PS.E)])
    b = runtime.Batch(D.compiled("c2"), PS.HP, PS.SEEDS, lib=lib, **kw)
    try:
        assert b.counters()["group_lanes"] == 16
        b.learn_begin()
        b.apply_qinit()
        for k in PS.SCHEDULES["c2"]:
            assert b.step(k)[0] == k * PS.E
        assert parity.check_batch(b, PS.HP, range(PS.E), PS.SCHEDULES["c2"], hostsim.lib(), **kw) == []
        assert not np.array_equal(b.q_raw(0)[0], b.q_raw(1)[0])
    finally:
        b.close()


def test_the_largest_map(lib, monkeypatch):
    """255 switches and 128 trains at G = 64 (k_wave2, two train slots per lane): tests/_shapes.py's row, chunks and
    hyperparameters (gamma 0.95, default_q -5, a decaying lr), every env against the host build."""
    monkeypatch.setenv("SFL_WAVE_G", "64")
    n = PS.big_envs()
    b = runtime.Batch(sh.compiled(PS.BIG), sh.HP, sh.seeds(n), lib=lib, ntab=sh.NTAB)
    try:
        cn = b.counters()
        assert (cn["kernel_variant"], cn["group_lanes"]) == (5, 64), cn
        b.learn_begin()
        b.apply_qinit()
        for k in sh.CHUNKS:
            assert b.step(k)[0] == k * n
        for e, (got, want) in enumerate(zip(sh.snapshot(b, n), sh.host_plain(PS.BIG, sh.CHUNKS, n))):
            assert not sh.same_env(got, want), f"env {e}: {sh.same_env(got, want)}"
    finally:
        b.close()


@pytest.mark.parametrize("S,T,expect", ((64, 32, (7, 16)), (16, 16, (6, 16))), ids=("v7", "c2-shape"))
def test_one_eval_batch_on_two_banks_in_turn(lib, monkeypatch, S, T, expect):
    """An evaluation, then the bank's tables replaced by their rotation and the same assignment evaluated again: each
    against the twin that was given those tables (MapDecide / MapLearn are read by the BANK kernels; bank_q stays where
    it was)."""
    monkeypatch.setenv("SFL_WAVE_G", "16")
    rw, n = EB.row(S, T), sh.n_envs(16)
    pol = EB.assign(n, "mod")
    ev = EB.bank(lib, rw, n, qf.MAX_STEPS)
    try:
        cn = ev.counters()
        assert (cn["kernel_variant"], cn["group_lanes"]) == expect, cn
        first = ev.evaluate(pol)
        bad = EB.mismatches(ev, first, EB.twin(rw, n, pol, qf.MAX_STEPS), pol)
        assert not bad, bad[:8]
        for p, tb in enumerate(EB.tables(rw)):
            ev.set_policy_raw((p - 1) % EB.P, *tb)  # bank[p] = table p + 1
        second = ev.evaluate(pol)
        bad = EB.mismatches(ev, second, EB.twin(rw, n, PS.rotated(pol), qf.MAX_STEPS), pol)
        assert not bad, bad[:8]
        assert not qf.same_bits(first["cum_reward"], second["cum_reward"])  # the other bank was followed
    finally:
        ev.close()


@pytest.mark.parametrize("c", [x for x in W.SWEEP if x.G == 16][:1] + [x for x in W.SWEEP if x.G == 64][:1], ids=W.case_id)
def test_external_action_mode_equals_the_host_build(lib, monkeypatch, c):
    monkeypatch.setenv("SFL_WAVE_G", str(c.G))
    got, ref = W.run(c, lib, "wave"), W.host_run(c)
    assert got["kernel"] == W.predict(c)
    assert W.mismatches(got, ref) == []


def test_a_small_partitioned_batch_equals_the_fused_one(lib, monkeypatch):
    """16 switches and 32 trains, block 0 of a 4-rank partition in place: tests/test_shape_edges_gpu.py's check."""
    case = next(c for c in sh.CASES if c.mode == "part" and c.row[:2] == (16, 32) and c.arg == "block0of4")
    edges.test_partitioned(lib, monkeypatch, case)
