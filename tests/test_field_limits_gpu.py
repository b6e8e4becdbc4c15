"""The wave kernels at their packed-field limits and counter wraps, on the MI355X (tests/_limits.py): the slot epoch's
wrap at resets 256 and 511 in every kernel family, the 32-bit semaphore record on and one past t_hi = 8191 and at a
span of 508 of at most 511, and the exploratory draw's Lemire rejection -- with the 2^31-entry table and without it
(SFL_SEEDSEQ_TABLE=0).  Every case runs E = 256 / G + 3 envs (two blocks, the second partly filled), asserts the
variant the engine reports, and compares every env with the host build of the lane body and sampled envs with the
oracle; tests/test_field_limits.py checks the host build against the oracle on the same runs."""
import functools
import importlib

import numpy as np
import pytest

from tests import _limits as lm
from tests import _shapes as sh
from tests.test_shape_edges_gpu import _OwnedRows, _all_envs_equal

pytestmark = pytest.mark.gpu

runtime = sh.runtime
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")
part = importlib.import_module("network-distributed-q-learning_amd.partition")

SWITCHES = ("SFL_KERNEL", "SFL_WAVE_G", "SFL_LDS_MAP", "SFL_REQUIRE_WAVE", "SFL_SEEDSEQ_TABLE")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


def _select(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _batch(case, lib, hp, seeds, key=None, **kw):
    """The case's device batch; fails unless it runs the kernel the case claims."""
    b = runtime.Batch(sh.compiled(key or case.row), hp, seeds, lib=lib, ntab=sh.NTAB, **kw)
    c = b.counters()
    want = lm.predict(case, key)
    assert (c["kernel_variant"], c["group_lanes"]) == want, (c, want)
    return b


def _ids(cases):
    return dict(argvalues=cases, ids=lm.case_id)


# ---- A. the epoch wrap ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", **_ids(lm.EPOCH_CASES))
def test_epoch_wrap_learn(lib, monkeypatch, case):
    """learn(600, exploit_freq=50) at max_steps = 7 (the TIMED kernel): 612 resets, the slot words cleared at resets
    256 and 511.  Every env's outputs, tables and state equal the host build's; the first and last env's outputs and Q
    dict the oracle's, whose resets are counted."""
    _select(monkeypatch, lm.case_env(case))
    n = sh.n_envs(case.G)
    b = _batch(case, lib, sh.HP, sh.seeds(n), max_steps=lm.EPOCH_MAX_STEPS)
    out = b.learn(**lm.EPOCH_LEARN)
    href, hsnap = lm.epoch_host_learn(case.row, n)
    for k in sh.LEARN_KEYS:
        assert np.array_equal(out[k], href[k][..., :n]), f"{k} vs the host build"
    _all_envs_equal(b, n, hsnap, "the host build")
    for e in (0, n - 1):
        ref = lm.epoch_oracle_learn(case.row, sh.seeds(n)[e])
        assert ref["resets"] >= lm.EPOCH_RESETS
        assert not lm.epoch_learn_mismatches(out, e, ref), f"env {e} vs the oracle"
        assert b.q_dict(e) == ref["q"], f"env {e} vs the oracle"
    if case.kernel is None:
        assert sum(b.phase_seconds().values()) > 0.0  # the phase-timed instantiation ran
    b.close()


def _oracle_wraps(row, seed, group=None):
    q, at = lm.epoch_oracle_plain(row, seed, group)
    assert len(at) >= lm.EPOCH_RESETS and at[lm.WRAPS[0] - 1] < lm.EPOCH_CHUNKS[0] < at[lm.WRAPS[0]]
    return q


@pytest.mark.parametrize("case", **_ids(lm.EPOCH_CASES))
def test_epoch_wrap_step(lib, monkeypatch, case):
    """sfl_step chunks (2044, 2200) at max_steps = 7 (the plain kernel, resets inside a launch): 531 episodes, the
    first chunk ending inside the episode that the first clearing reset begins.  Every env equal to the host build,
    the first and last env's Q dict to the oracle's."""
    _select(monkeypatch, lm.case_env(case))
    n = sh.n_envs(case.G)
    b = _batch(case, lib, sh.HP, sh.seeds(n), max_steps=lm.EPOCH_MAX_STEPS)
    b.learn_begin()
    b.apply_qinit()
    for k in lm.EPOCH_CHUNKS:
        assert b.step(k)[0] == k * n
    _all_envs_equal(b, n, lm.epoch_host_plain(case.row, n), "the host build")
    for e in (0, n - 1):
        assert b.q_dict(e) == _oracle_wraps(case.row, sh.seeds(n)[e]), f"env {e} vs the oracle"
    b.close()


def test_epoch_wrap_hparam_groups(lib, monkeypatch):
    """The same chunks through the hyperparameter-group instantiation: every env equal to the grouped host build, the
    last env of each group to the oracle run with that group's hyperparameters."""
    case = lm.EPOCH_HPG
    _select(monkeypatch, lm.case_env(case))
    n = sh.n_envs(case.G)
    b = _batch(case, lib, sh.HANDLE_HP, sh.hpg_seeds(n), hparam_groups=sh.GROUPS, env_group=sh.env_groups(n),
               max_steps=lm.EPOCH_MAX_STEPS)
    b.learn_begin()
    b.apply_qinit()
    for k in lm.EPOCH_CHUNKS:
        assert b.step(k)[0] == k * n
    _all_envs_equal(b, n, sh.host_hpg(case.row, n, lm.EPOCH_CHUNKS, lm.EPOCH_MAX_STEPS), "the grouped host build")
    for e in (n - 2, n - 1):
        assert b.q_dict(e) == _oracle_wraps(case.row, sh.hpg_seeds(n)[e], e % 2), f"env {e} (group {e % 2})"
    assert not np.array_equal(b.q_raw(0)[0], b.q_raw(1)[0])
    b.close()


def test_epoch_wrap_partitioned(lib, monkeypatch):
    """The same chunks through the partitioned local step, every row operation a message (the epoch travels in
    eblk[EB_EPOCH]): owned rows, key sets and env states of every env equal to the fused HIP batch, the first and last
    env's rows to the oracle.  (PartitionedBatch passes no max_steps on: its batch is made with max_steps = 7 here.)"""
    import torch
    case = lm.EPOCH_PART
    _select(monkeypatch, lm.case_env(case))
    cm, n = sh.compiled(case.row), sh.n_envs(case.G)
    fused = _batch(case, lib, sh.HP, sh.seeds(n), max_steps=lm.EPOCH_MAX_STEPS)
    fused.learn_begin()
    fused.apply_qinit()
    monkeypatch.setattr(part, "Batch", functools.partial(runtime.Batch, max_steps=lm.EPOCH_MAX_STEPS))
    pb = part.PartitionedBatch(cm, sh.HP, sh.seeds(n), 0, n, lib=lib, ntab=sh.NTAB, buffer_device="cuda", local_rows=False)
    c = pb.batch.counters()
    assert (c["kernel_variant"], c["group_lanes"]) == (sh.wave64_variant(cm.S, cm.T), 64), c
    pb.learn_begin()
    pb.apply_qinit()
    for k in lm.EPOCH_CHUNKS:
        fused.step(k)
        assert pb.step(k) >= k  # (a round per decision, every row operation a message)
    torch.cuda.synchronize()
    assert pb.owned_mask().all()
    for e in range(n):
        got = pb.owned_q(e) + (sh.parity.env_state(*pb.sim_env(e)),)
        want = fused.q_raw(e) + (sh.parity.env_state(fused, e),)
        assert not sh.same_env(got, want), f"env {e} vs the fused batch: {sh.same_env(got, want)}"
    _all_envs_equal(fused, n, lm.epoch_host_plain(case.row, n), "the host build")
    rows = _OwnedRows(pb)
    for e in (0, n - 1):
        assert rows.q_dict(e) == _oracle_wraps(case.row, sh.seeds(n)[e]), f"env {e}"
    pb.close()
    fused.close()


# ---- B. the semaphore record's limits -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", **_ids(lm.HORIZON_CASES))
def test_horizon_on_the_limit_learn(lib, monkeypatch, case):
    """t_hi == 8191, a third of the trains departing in the episode's last ~100 ticks: full episodes of ~8,160 ticks,
    every env's outputs, tables and state (semaphores included) equal to the host build's, the last env's outputs and
    Q dict to the oracle's."""
    _select(monkeypatch, lm.case_env(case))
    key, n, learn = lm.horizon_key(case.row), sh.n_envs(case.G), lm.HORIZON_LEARN[case.row[:2]]
    assert lm.span_and_t_hi(sh.compiled(key), sh.scenario(key))[1] == lm.T_HI_MAX
    b = _batch(case, lib, sh.HP, sh.seeds(n), key)
    assert b.kernel_note == ""
    out = b.learn(**learn)
    href, hsnap = sh.host_learn(key, 100_000, n, **learn)
    assert href["ticks"].max() == sh.scenario(key).max_episode_steps
    for k in sh.LEARN_KEYS:
        assert np.array_equal(out[k], href[k][..., :n]), f"{k} vs the host build"
    _all_envs_equal(b, n, hsnap, "the host build")
    ref = sh.oracle_learn(key, sh.seeds(n)[n - 1], 100_000, False, **learn)
    assert not sh.learn_mismatches(out, n - 1, ref, **learn), "last env vs the oracle"
    assert b.q_dict(n - 1) == ref["q"]
    b.close()


@pytest.mark.parametrize("case", **_ids(lm.HORIZON_CASES))
def test_horizon_on_the_limit_step(lib, monkeypatch, case):
    """sfl_step chunks chosen from the host build's run: at the second snapshot envs stand past tick 8000 of their
    first episode and hold present records with t0 >= 4096 -- the 14-bit field's top bit -- which is asserted on the
    host build's state; every env's tables and state (semaphores included) equal the host build's at that snapshot."""
    _select(monkeypatch, lm.case_env(case))
    key, n, chunks = lm.horizon_key(case.row), sh.n_envs(case.G), lm.HORIZON_CHUNKS[case.row[:2]]
    snaps, seen = lm.host_stepped_snapshots(key, chunks, n)
    late = [e for e, s in enumerate(snaps[1])
            if s[2][0] > 8000 and (lm.sem_fields(s[2][2])[1][lm.sem_fields(s[2][2])[0]] >= 4096).any()]
    print(f"envs past tick 8000 holding a record of t0 >= 4096: {late}; largest t0 {seen[1][1]}")
    assert late and seen[1][1] >= 4096
    b = _batch(case, lib, sh.HP, sh.seeds(n), key)
    b.learn_begin()
    b.apply_qinit()
    for k, snap in zip(chunks, snaps):
        assert b.step(k)[0] == k * n
        _all_envs_equal(b, n, snap, "the host build")
    b.close()


def _refused(lib, monkeypatch, case, key, note):
    """A map one past a limit: the lane-per-env kernel with the note and a warning, refused under SFL_REQUIRE_WAVE=1,
    and k_run's result bit-equal to the host build."""
    _select(monkeypatch, lm.case_env(case))
    n, cm = sh.n_envs(case.G), sh.compiled(key)
    with pytest.warns(RuntimeWarning, match=note):
        b = runtime.Batch(cm, sh.HP, sh.seeds(n), lib=lib, ntab=sh.NTAB)
    assert b.counters()["kernel_variant"] == 0 and b.kernel_note == note
    b.learn_begin()
    b.apply_qinit()
    for k in sh.CHUNKS:
        assert b.step(k)[0] == k * n
    _all_envs_equal(b, n, sh.host_plain(key, sh.CHUNKS, n), "the host build")
    b.close()
    monkeypatch.setenv("SFL_REQUIRE_WAVE", "1")
    with pytest.raises(_lib.SflError, match=note):
        runtime.Batch(cm, sh.HP, sh.seeds(n), lib=lib, ntab=sh.NTAB)


@pytest.mark.parametrize("case", **_ids(lm.HORIZON_CASES))
def test_horizon_one_past_the_limit(lib, monkeypatch, case):
    key = lm.horizon_key(case.row, 1)
    assert lm.span_and_t_hi(sh.compiled(key), sh.scenario(key))[1] == lm.T_HI_MAX + 1
    _refused(lib, monkeypatch, case, key, lm.NOTE_HORIZON)


@pytest.mark.parametrize("G", lm.SPAN_GS)
def test_span_under_the_limit(lib, monkeypatch, G):
    """Span 508 of at most 511 (the nearest the generator reaches): records of a duration beyond 255 ticks -- the
    9-bit field's top bit -- are present at both snapshots of the host build; every env equal to it at both, the last
    env's Q dict to the oracle's."""
    case, key = lm.Case(None, G, None), lm.span_key(lm.SPAN_ON)
    _select(monkeypatch, lm.case_env(case))
    n = sh.n_envs(G)
    assert lm.span_and_t_hi(sh.compiled(key), sh.scenario(key))[0] == 508
    snaps, seen = lm.host_stepped_snapshots(key, lm.SPAN_CHUNKS, n)
    print("largest (duration, t0) at each snapshot of the host build:", seen)
    assert all(255 < d <= lm.SPAN_MAX for d, _ in seen)
    b = _batch(case, lib, sh.HP, sh.seeds(n), key)
    assert b.kernel_note == ""
    b.learn_begin()
    b.apply_qinit()
    for k, snap in zip(lm.SPAN_CHUNKS, snaps):
        assert b.step(k)[0] == k * n
        _all_envs_equal(b, n, snap, "the host build")
    assert b.q_dict(n - 1) == lm.oracle_stepped(key, sh.seeds(n)[n - 1], sum(lm.SPAN_CHUNKS))[0]
    b.close()


def test_span_one_past_the_limit(lib, monkeypatch):
    key = lm.span_key(lm.SPAN_PAST)
    assert lm.span_and_t_hi(sh.compiled(key), sh.scenario(key))[0] == 512
    _refused(lib, monkeypatch, lm.Case(None, 64, None), key, lm.NOTE_SPAN)


# ---- C. the rejected exploratory draw, and a device without the table ----------------------------------------------
def _draw(lib, case):
    """step(20) from the crafted states at epsilon = 1: every env's first decision explores with its sub-seed (the two
    rejecting ones and the controls, cycled over the envs)."""
    n = sh.n_envs(case.G)
    b = _batch(case, lib, lm.HP_EXPLORE, sh.seeds(n))
    lm.draw_run(b, lm.draw_states(sh.seeds(n)))
    _all_envs_equal(b, n, lm.host_draw(case.row, n), "the host build")
    for e, v in enumerate(lm.REJECTING):
        ref = lm.oracle_draw(case.row, sh.seeds(n)[e], v)
        allowed = np.nonzero(ref["mask"])[0]
        assert len(allowed) == 3 and ref["action"] == allowed[2]  # the rejection's pick; without it, allowed[0]
        assert b.q_dict(e) == ref["q"], f"env {e} (sub-seed {v}) vs the oracle"
    b.close()


@pytest.mark.parametrize("case", **_ids(lm.DRAW_CASES))
def test_rejected_draw(lib, monkeypatch, case):
    """Every env equal to the host build given the same states; the envs of the two rejecting sub-seeds equal to the
    oracle, whose first decision has three allowed actions and takes the third."""
    _select(monkeypatch, lm.case_env(case))
    _draw(lib, case)


def test_rejected_draw_hparam_groups(lib, monkeypatch):
    case = lm.DRAW_HPG
    _select(monkeypatch, lm.case_env(case))
    n = sh.n_envs(case.G)
    b = _batch(case, lib, sh.HANDLE_HP, sh.seeds(n), hparam_groups=lm.GROUPS_EXPLORE, env_group=sh.env_groups(n))
    lm.draw_run(b, lm.draw_states(sh.seeds(n)))
    _all_envs_equal(b, n, lm.host_draw(case.row, n, True), "the grouped host build")
    for e, v in enumerate(lm.REJECTING):
        ref = lm.oracle_draw(case.row, sh.seeds(n)[e], v, e % 2)
        assert ref["action"] == np.nonzero(ref["mask"])[0][2] and ref["mask"].sum() == 3
        assert b.q_dict(e) == ref["q"], f"env {e} (group {e % 2}) vs the oracle"
    b.close()


def test_rejected_draw_partitioned(lib, monkeypatch):
    """The partitioned local step, every row operation a message: the draw happens in the observe-only step."""
    import torch
    case = lm.DRAW_PART
    _select(monkeypatch, lm.case_env(case))
    cm, n = sh.compiled(case.row), sh.n_envs(case.G)
    pb = part.PartitionedBatch(cm, lm.HP_EXPLORE, sh.seeds(n), 0, n, lib=lib, ntab=sh.NTAB, buffer_device="cuda",
                               local_rows=False)
    c = pb.batch.counters()
    assert (c["kernel_variant"], c["group_lanes"]) == (sh.wave64_variant(cm.S, cm.T), 64), c
    lm.learn_begin_with(pb.batch, lm.draw_states(sh.seeds(n)))
    pb.apply_qinit()
    assert pb.step(lm.DRAW_STEPS) >= lm.DRAW_STEPS
    torch.cuda.synchronize()
    assert pb.owned_mask().all()
    for e, want in enumerate(lm.host_draw(case.row, n)):
        got = pb.owned_q(e) + (sh.parity.env_state(*pb.sim_env(e)),)
        assert not sh.same_env(got, want), f"env {e} vs the host build: {sh.same_env(got, want)}"
    rows = _OwnedRows(pb)
    for e, v in enumerate(lm.REJECTING):
        assert rows.q_dict(e) == lm.oracle_draw(case.row, sh.seeds(n)[e], v)["q"], f"env {e} (sub-seed {v})"
    pb.close()


@pytest.mark.parametrize("case", lm.NO_TABLE_CASES, ids=sh.case_id)
def test_no_table_plain(lib, monkeypatch, case):
    """SFL_SEEDSEQ_TABLE=0, a device that could not allocate the table: every exploratory draw runs the sub-generator.
    The plain sweep case of tests/test_shape_edges_gpu.py, one per kernel family, against the same references."""
    _select(monkeypatch, dict(sh.case_env(case), SFL_SEEDSEQ_TABLE="0"))
    n = sh.n_envs(case.G)
    b = runtime.Batch(sh.compiled(case.row), sh.HP, sh.seeds(n), lib=lib, ntab=sh.NTAB)
    c = b.counters()
    assert (c["kernel_variant"], c["group_lanes"]) == sh.predict(case), (c, sh.predict(case))
    b.learn_begin()
    b.apply_qinit()
    for k in sh.CHUNKS:
        assert b.step(k)[0] == k * n
    _all_envs_equal(b, n, sh.host_plain(case.row, sh.CHUNKS, n), "the host build")
    for e in (0, n - 1):
        assert b.q_dict(e) == sh.oracle_plain(case.row, sh.seeds(n)[e]), f"env {e} vs the oracle"
    b.close()


@pytest.mark.parametrize("case", **_ids(lm.NO_TABLE_DRAW))
def test_no_table_rejected_draw(lib, monkeypatch, case):
    _select(monkeypatch, dict(lm.case_env(case), SFL_SEEDSEQ_TABLE="0"))
    _draw(lib, case)
