"""The tick's semaphore pass on the MI355X: one pass over each lane's records that deletes those of the trains that
became done in the tick (not of every done train on every tick) and retimes those of stopped and malfunctioning
trains.  What the recorded goldens reach only by luck, with malfunctions frequent (rate 0.2, 2-6 ticks): an arrival
followed by many further ticks of its episode, an arrival and a stopped or malfunctioning train in one tick, episodes
ended at max_episode_steps with trains still on the map, and launch boundaries between an arrival and the next tick
(the done flag travels through store() / load()).  Every env of every case is compared with the host build through
parity.check_batch: Q-table, key set and env state, the semaphore records included; the external-action case compares
every output of every call and the final env states.  tests/_sempass.py has the cases and asserts nothing vacuous."""
import importlib

import numpy as np
import pytest

from tests import _aec_wave as W, _sempass as S, hostsim

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


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_every_env_equals_the_host_build(lib, monkeypatch, c):
    if c.G is not None:
        monkeypatch.setenv("SFL_WAVE_G", str(c.G))
    cm = S.compiled(c.cfg, c.mes)
    S.check_reference(c)
    b = runtime.Batch(cm, S.HP, S.SEEDS, lib=lib, ntab=S.NTAB)
    try:
        cn = b.counters()
        assert cn["kernel_variant"] > 0 and cn["group_lanes"] == c.lanes, cn
        if c.cfg == "c3" and c.G == 16:
            assert cn["kernel_variant"] == 7, cn
        b.learn_begin()
        b.apply_qinit()
        for n in c.schedule:
            got, _ = b.step(n)
            assert got == n * S.E
        assert parity.check_batch(b, S.HP, range(S.E), c.schedule, hostsim.lib(), ntab=S.NTAB) == []
    finally:
        b.close()


def test_external_actions_on_the_wave_kernel(lib, monkeypatch):
    """c2 in external-action mode (sfl_env_begin_wave, G = 16): the same tick() under the EXT driver."""
    monkeypatch.setenv("SFL_WAVE_G", "16")
    cm = S.compiled("c2")
    c = W.Case(None, 16)
    got = W.run(c, lib, "wave", cm=cm, seeds=S.SEEDS)
    ref = W.run(c, hostsim.lib(), "lane", cm=cm, seeds=S.SEEDS)
    assert got["kernel"][0] > 0 and got["kernel"][1] == 16, got["kernel"]
    assert W.episode_ends(ref) >= 2 * S.E
    # a train arrived and its env went on to a later call
    assert any(np.logical_and(o["arrived"] != 0, o["agent"] >= 0).any() for o in ref["outs"])
    assert W.mismatches(got, ref) == []
