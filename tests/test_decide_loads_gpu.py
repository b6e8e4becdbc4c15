"""decide()'s epsilon load issued ahead of the observation and post()'s pending row recomputed from the port record,
on the MI355X.  Neither may change a result: every env of every case equals the host build -- Q-table, key set, env
state, and after every launch the five stored words of its epsilon-greedy stream -- over schedules that put
one-decision launches between launches of a few hundred decisions, so the stream's has / buf half is stored and
reloaded inside a pair of draws.  tests/_decide_loads.py has the cases (all exploring, none exploring, greedy rounds
between learning ones, a table shorter than the run, no sub-generator table, Lemire's rejected draws, hyperparameter
groups that differ in epsilon); tests/test_decide_loads.py asserts that none is vacuous.  The policy-bank and
external-action kernels, which keep their order, against their twins."""
import importlib

import numpy as np
import pytest

from tests import _aec_wave as W, _decide_loads as D, _evalbank as EB, hostsim

pytestmark = pytest.mark.gpu

runtime = importlib.import_module("network-distributed-q-learning_amd.runtime")
parity = importlib.import_module("network-distributed-q-learning_amd.parity")
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")

SWITCHES = ("SFL_KERNEL", "SFL_WAVE_G", "SFL_LDS_MAP", "SFL_REQUIRE_WAVE", "SFL_ENV_KERNEL", "SFL_SEEDSEQ_TABLE")
# the conditions parity.check_batch can drive itself (learn_begin, the optimistic init, the schedule)
PLAIN = ("base", "eps1", "eps0", "short", "notable", "hpg")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_every_env_equals_the_host_build(lib, monkeypatch, c):
    for k, v in D.env_vars(c).items():
        monkeypatch.setenv(k, v)
    ref, sch = D.ref_of(c), D.schedule(c)
    b = runtime.Batch(D.compiled(c.cfg), D.HPS[c.cond], D.SEEDS, lib=lib, **D.kwargs(c))
    try:
        cn = b.counters()
        assert cn["kernel_variant"] > 0 and cn["group_lanes"] == c.lanes, cn
        if c.cfg in ("c3", "rej") and c.G == 16:
            assert cn["kernel_variant"] == 7, cn
        D.start(b, c)
        assert np.array_equal(D.stream_words(b), ref.streams[0])
        for i, k in enumerate(sch):
            got, _ = b.step(k)
            assert got == ref.decisions[i]
            w = D.stream_words(b)
            bad = np.nonzero((w != ref.streams[i + 1]).any(axis=1))[0]
            assert not len(bad), f"launch {i} ({k} decisions): the stream words of envs {bad[:8].tolist()} differ"
        assert D.mismatches(D.snapshot(b), ref.final) == []
        if c.cond in PLAIN:
            assert parity.check_batch(b, D.HPS[c.cond], range(D.E), sch, hostsim.lib(), **D.kwargs(c)) == []
    finally:
        b.close()


def test_policy_bank_equals_the_twin(lib, monkeypatch):
    """EvalBatch (the BANK kernels: no draw, no epsilon) against test(1) of a twin batch on the host build, G = 16."""
    monkeypatch.setenv("SFL_WAVE_G", "16")
    EB.run_twin_equality(lib, EB.row(16, 16), EB.sh.n_envs(16), expect=(6, 16))


def test_external_action_mode_equals_the_host_build(lib, monkeypatch):
    """One EXT cell of the launch table at G = 16 against the host build's lane-per-env body: every output of every
    call, the launch counters and the final env state."""
    c = next(x for x in W.SWEEP if x.G == 16)
    monkeypatch.setenv("SFL_WAVE_G", str(c.G))
    got, ref = W.run(c, lib, "wave"), W.host_run(c)
    assert got["kernel"] == W.predict(c)
    assert W.mismatches(got, ref) == []
