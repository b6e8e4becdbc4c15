"""Consensus Q-tables (sfl_consensus / sfl_get_consensus_q) on the host build: every case of tests/_consensus.py
against the numpy model of the merge rule, bit for bit, and learning that goes on from shared tables.
tests/test_consensus_gpu.py runs the same cases on the MI355X."""
import importlib
import pickle

import numpy as np
import pytest

from tests import _consensus as cs
from tests import hostsim
from tests import _shapes as sh

env_mod = importlib.import_module("network-distributed-q-learning_amd.env")
distr_q = importlib.import_module("network-distributed-q-learning_amd.distr_q")


@pytest.mark.parametrize("case", list(cs.CASES))
def test_case(case):
    cs.CASES[case](hostsim.lib())


@pytest.mark.parametrize("name", cs.CONTINUE_MAPS)
def test_continue_sharing_reaches_a_decision(name):
    """step(40), consensus(share) with two cohorts, step(40): the members of a cohort leave the sync with one table,
    and at least one env's state after the second step (trains, semaphores, clock: what its decisions made of it)
    differs from the same run without the sync -- asserted on c1 (two trains); on the one-train map the 40 decisions
    after the sync leave every env's state as without it, and only the tables differ."""
    with_sync, without = cs.host_continue(name, True), cs.host_continue(name, False)
    differs = [e for e in range(cs.CONTINUE_E)
               if [p for p in sh.same_env(with_sync[e], without[e]) if p not in ("Q-table", "key set")]]
    assert differs or name != "c1", "no env decided differently after the sync"
    assert all("Q-table" in sh.same_env(with_sync[e], without[e]) for e in range(cs.CONTINUE_E))


def test_save_consensus_round_trips_through_load(tmp_path):
    """DistrQLearning.save(consensus="mean") writes cohort 0's consensus table in the reference's pickle format: one
    dict, which load puts into every env; save's default is unchanged (a list of the envs' dicts)."""
    lib = hostsim.lib()
    env = env_mod.ASyncSwitchEnv(sh.scenario(cs._owner.ROW), n_envs=5)
    dq = distr_q.DistrQLearning(env, gamma=0.95, epsilon=0.3, epsilon_decay_rate=0.99, lr=0.2, lr_decay_rate=0.999,
                                default_q=-5.0, lib=lib)
    b = dq.batch
    b.learn_begin()
    b.apply_qinit()
    b.step(60)
    before = [b.q_raw(e) for e in range(5)]
    f_plain, f_cons = str(tmp_path / "q.pkl"), str(tmp_path / "consensus.pkl")
    dq.save(f_plain)
    dq.save(f_cons, consensus="mean")
    plain, cons = pickle.load(open(f_plain, "rb")), pickle.load(open(f_cons, "rb"))
    assert isinstance(plain, list) and plain == [b.q_dict(e) for e in range(5)]
    assert isinstance(cons, dict) and cons == dq.consensus_table("mean") and len(cons) >= max(len(t) for t in plain)
    for e in range(5):  # saving shared nothing
        assert np.array_equal(before[e][0].view(np.uint64), b.q_raw(e)[0].view(np.uint64))
    table = dq.consensus_table("mean", share=True)
    shared = b.q_raw(0)
    dq.load(f_cons)
    for e in range(5):
        assert b.q_dict(e) == cons == table
        assert np.array_equal(b.q_raw(e)[1], shared[1])
    b.close()
