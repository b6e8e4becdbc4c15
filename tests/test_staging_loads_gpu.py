"""The Q loads the batch staging issues together (prefetch_slot(): the pending update's cell first, then the staged
row's clamped columns, held in front of the reduction), on the MI355X.  It may not change a result: every env of every
case is compared with the host build through parity.check_batch (Q-table, key set and env state) over a schedule that
mixes one-decision launches with launches of a few hundred decisions, with malfunctions frequent (rate 0.2, 2-6 ticks)
so that batches of several queued trains occur; the policy-bank case (no pending cell) against test(1) of a twin
batch.  The cases run every family that stages Q values: G = 8 / 16 / 32 / 64, variant 7, two train slots per lane
(128 trains), the Flatland malfunction stream, the bank, and a small map at delay_threshold 0 on which the last env
decides at the last row of its Q block.  tests/_staging.py has the cases and asserts nothing vacuous."""
import importlib

import pytest

from tests import _evalbank as EB, _staging as T, hostsim

pytestmark = pytest.mark.gpu

runtime = importlib.import_module("network-distributed-q-learning_amd.runtime")
parity = importlib.import_module("network-distributed-q-learning_amd.parity")
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in ("SFL_KERNEL", "SFL_WAVE_G", "SFL_LDS_MAP", "SFL_REQUIRE_WAVE", "SFL_ENV_KERNEL"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_every_env_equals_the_host_build(lib, monkeypatch, c):
    if c.G is not None:
        monkeypatch.setenv("SFL_WAVE_G", str(c.G))
    T.check_reference(c)
    n = T.n_envs(c)
    b = runtime.Batch(T.compiled(c.cfg), T.HP, T.seeds(c), lib=lib, **T.kwargs(c))
    try:
        cn = b.counters()
        assert cn["kernel_variant"] > 0 and cn["group_lanes"] == c.lanes, cn
        if c.cfg == "c3" and c.G == 16:
            assert cn["kernel_variant"] == 7, cn
        b.learn_begin()
        b.apply_qinit()
        for k in c.schedule:
            got, _ = b.step(k)
            assert got == k * n
        assert parity.check_batch(b, T.HP, range(n), c.schedule, hostsim.lib(), **T.kwargs(c)) == []
    finally:
        b.close()


def test_policy_bank_equals_the_twin(lib, monkeypatch):
    """EvalBatch (the BANK kernels: the staged row comes from a shared table, no pending cell) against test(1) of a twin
    batch on the host build, G = 16."""
    monkeypatch.setenv("SFL_WAVE_G", "16")
    EB.run_twin_equality(lib, EB.row(16, 16), EB.sh.n_envs(16), expect=(6, 16))
