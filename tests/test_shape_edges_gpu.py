"""Every wave-kernel shape at the edges of its envelope, on the MI355X: each case of tests/_shapes.py CASES runs one
(edge row, group size, instantiation) -- the plain, TRACE, TIMED and hyperparameter-group kernels of variants 1 - 11
and the partitioned local step of variants 1 - 5 -- on E = 256 / G + 3 envs (two blocks, the second partly filled; the
traced and sampled env is the last one), asserts the variant the engine reports is the one the case claims, and
compares every env with the host build of the lane body and sampled envs with the oracle.  The references are
tests/_shapes.py's, computed once per (row, mode); tests/test_shape_edges.py checks host build against oracle and
that the cases cover the (variant x instantiation) matrix."""
import importlib

import numpy as np
import pytest

from tests import _shapes as sh
from tests import _trace

pytestmark = pytest.mark.gpu

runtime = sh.runtime
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")
part = importlib.import_module("network-distributed-q-learning_amd.partition")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


def _select(monkeypatch, case):
    for k in ("SFL_KERNEL", "SFL_WAVE_G", "SFL_LDS_MAP", "SFL_REQUIRE_WAVE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in sh.case_env(case).items():
        monkeypatch.setenv(k, v)


def _batch(case, lib, hp, seeds, **kw):
    """The case's device batch; fails unless it runs the kernel the case claims."""
    b = runtime.Batch(sh.compiled(case.row), hp, seeds, lib=lib, ntab=sh.NTAB, **kw)
    c = b.counters()
    assert (c["kernel_variant"], c["group_lanes"]) == sh.predict(case), (c, sh.predict(case))
    return b


def _all_envs_equal(b, n, ref, what):
    for e, (got, want) in enumerate(zip(sh.snapshot(b, n), ref)):
        assert not sh.same_env(got, want), f"env {e} vs {what}: {sh.same_env(got, want)}"


def _cases(*modes):
    cs = [c for c in sh.CASES if c.mode in modes]
    return pytest.mark.parametrize("case", cs, ids=sh.case_id)


@_cases("plain")
def test_plain(lib, monkeypatch, case):
    """sfl_step in chunks [50, 130]: Q-table, key set and env state of every env bit-equal to the host build; the
    first and the last env equal to the oracle."""
    _select(monkeypatch, case)
    n = sh.n_envs(case.G)
    b = _batch(case, lib, sh.HP, sh.seeds(n))
    b.learn_begin()
    b.apply_qinit()
    for k in sh.CHUNKS:
        assert b.step(k)[0] == k * n
    _all_envs_equal(b, n, sh.host_plain(case.row, sh.CHUNKS, n), "the host build")
    for e in (0, n - 1):
        assert b.q_dict(e) == sh.oracle_plain(case.row, sh.seeds(n)[e]), f"env {e} vs the oracle"
    b.close()


def _learn(case, lib, trace, max_steps=100_000):
    n = sh.n_envs(case.G)
    b = _batch(case, lib, sh.HP, sh.seeds(n), max_steps=max_steps)
    b.trace_env = n - 1 if trace else None
    out = b.learn(sh.LEARN["n_episodes"], exploit_freq=sh.LEARN["exploit_freq"])
    href, hsnap = sh.host_learn(case.row, max_steps, n)
    for k in sh.LEARN_KEYS:
        assert np.array_equal(out[k], href[k][..., :n]), f"{k} vs the host build"
    _all_envs_equal(b, n, hsnap, "the host build")
    ref = sh.oracle_learn(case.row, sh.seeds(n)[n - 1], max_steps, trace)
    assert not sh.learn_mismatches(out, n - 1, ref), "last env vs the oracle"
    assert b.q_dict(n - 1) == ref["q"]
    return b, ref


@_cases("timed")
def test_timed(lib, monkeypatch, case):
    """learn(2, exploit_freq=2), untraced (the TIMED kernel), across episode ends, resets and an exploit episode:
    every env's outputs equal to the host build's, the last env's and its Q dict to the oracle's."""
    _select(monkeypatch, case)
    b, _ = _learn(case, lib, trace=False)
    assert sum(b.phase_seconds().values()) > 0.0  # the phase-timed instantiation ran
    b.close()


@_cases("trace")
def test_trace(lib, monkeypatch, case):
    """The same learn with the last env traced (the TRACE kernel): its decoded per-decision records equal the
    oracle's, as test_gpu.py::test_golden_env0_and_trace compares them."""
    _select(monkeypatch, case)
    b, ref = _learn(case, lib, trace=True)
    assert sum(b.phase_seconds().values()) == 0.0  # the trace instantiation carries no timers
    assert len(ref["recs"]) > sum(ref["decisions"])  # (the exploit episode's decisions are traced too)
    assert _trace.decode_kernel_trace(b.last_trace) == ref["recs"]
    b.close()


@_cases("trunc")
def test_truncation(lib, monkeypatch, case):
    """max_steps below the episode length: every episode is cut after max_steps + 1 decisions with trains under way
    (asserted on the oracle's outputs); outputs and tables as in test_timed."""
    _select(monkeypatch, case)
    b, ref = _learn(case, lib, trace=False, max_steps=case.arg)
    assert ref["decisions"] == [case.arg + 1] * sh.LEARN["n_episodes"]
    assert max(ref["out"]["arrived_trains"]) < case.row[1]
    b.close()


@_cases("hpg")
def test_hparam_groups(lib, monkeypatch, case):
    """Two hyperparameter groups interleaved e % 2, envs 2 i and 2 i + 1 on one seed: every env bit-equal to the
    grouped host build, the last env of each group to the oracle run with that group's hyperparameters; the two groups'
    tables differ."""
    _select(monkeypatch, case)
    n = sh.n_envs(case.G)
    b = _batch(case, lib, sh.HANDLE_HP, sh.hpg_seeds(n), hparam_groups=sh.GROUPS, env_group=sh.env_groups(n))
    b.learn_begin()
    b.apply_qinit()
    for k in sh.CHUNKS:
        assert b.step(k)[0] == k * n
    _all_envs_equal(b, n, sh.host_hpg(case.row, n), "the grouped host build")
    for e in (n - 2, n - 1):
        assert b.q_dict(e) == sh.oracle_plain(case.row, sh.hpg_seeds(n)[e], e % 2), f"env {e} (group {e % 2})"
    assert not np.array_equal(b.q_raw(0)[0], b.q_raw(1)[0])
    b.close()


class _OwnedRows:
    """A partitioned batch's rows read as runtime.Batch.q_dict reads a batch's."""
    q_dict = runtime.Batch.q_dict

    def __init__(self, pb):
        self.pb, self.cm, self.hp = pb, pb.cm, pb.batch.hp

    def q_raw(self, e):
        return self.pb.owned_q(e)


@_cases("part")
def test_partitioned(lib, monkeypatch, case):
    """partition.PartitionedBatch on one rank with device buffers, steps (40, 75), every row operation a message or
    block 0 of a 4-rank partition in place: owned rows and key sets of every env bit-equal to the fused HIP batch, env
    states too, and the first and last env's rows equal to the oracle directly."""
    import torch
    _select(monkeypatch, case)
    cm, n = sh.compiled(case.row), sh.n_envs(case.G)
    fused = _batch(case._replace(mode="plain"), lib, sh.HP, sh.seeds(n))
    fused.learn_begin()
    fused.apply_qinit()
    loc = (part.partition_switches(cm, 4) == 0).astype(np.uint8) if case.arg == "block0of4" else case.arg
    pb = part.PartitionedBatch(cm, sh.HP, sh.seeds(n), 0, n, lib=lib, ntab=sh.NTAB, buffer_device="cuda", local_rows=loc)
    c = pb.batch.counters()
    assert (c["kernel_variant"], c["group_lanes"]) == sh.predict(case), c
    pb.learn_begin()
    pb.apply_qinit()
    for k in sh.PART_STEPS:
        fused.step(k)
        rounds = pb.step(k)
        assert rounds == k + 1 if case.arg is False else 1 < rounds <= k + 1
    torch.cuda.synchronize()
    assert pb.owned_mask().all()
    for e in range(n):
        got = pb.owned_q(e) + (sh.parity.env_state(*pb.sim_env(e)),)
        want = fused.q_raw(e) + (sh.parity.env_state(fused, e),)
        assert not sh.same_env(got, want), f"env {e} vs the fused batch: {sh.same_env(got, want)}"
    rows = _OwnedRows(pb)
    for e in (0, n - 1):
        assert rows.q_dict(e) == sh.oracle_plain(case.row, sh.seeds(n)[e], None, sum(sh.PART_STEPS)), f"env {e}"
    pb.close()
    fused.close()
