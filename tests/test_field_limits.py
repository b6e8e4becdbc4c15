"""The field-limit sweep without a GPU: the constants tests/_limits.py rests on read from the headers, the scenarios
on and one past the semaphore record's limits, the crafted generator states, and the reference side of every
comparison tests/test_field_limits_gpu.py makes -- the host build of the lane body against the oracle.

Sensitivity of the epoch-wrap cases (checked once, with mutants of sfl_core.h env_reset that are not committed): with
the clear loop deleted, cut to i < S T / 2 or cut to i >= S T / 2, the host build fails the learn comparison below
(cum_reward, from an episode between 281 and 591) on every row of EPOCH_ROWS, in the first and in the last env; the Q
dicts differ in 2 of the 8 rows only, which is why the learn outputs are compared."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _limits as lm
from tests import _shapes as sh
from tests import hostsim
from tests.test_shape_edges import _src

runtime = sh.runtime


# ---- the constants, from the headers ----------------------------------------------------------------------------
def test_constants_equal_the_headers():
    core = re.sub(r"\s+", "", _src("sfl_core.h"))
    # 8 epoch bits, the top byte of a slot word, in slot_make / slot_pend / slot_rew
    assert "((uint64_t)(epoch&0xFFu)<<56)" in core
    assert core.count("(uint32_t)(v>>56)==(epoch&0xFFu)") + core.count("(uint32_t)(v>>56)!=(epoch&0xFFu)") == 2
    assert "v.epoch=(v.epoch+1u)&0xFFu;if(v.epoch==0){" in core  # env_reset: the clear when the epoch passes 0
    assert lm.EPOCH_BITS == 8 and lm.WRAPS == (256, 511)
    m = re.search(r"constexpruint32_tR_T0_BITS=(\d+),R_DUR_BITS=(\d+),R_OWNER_SHIFT=R_T0_BITS\+R_DUR_BITS;", core)
    assert (int(m.group(1)), int(m.group(2))) == (lm.R_T0_BITS, lm.R_DUR_BITS) == (14, 9)
    assert "R_DUR_MASK=(1u<<R_DUR_BITS)-1u" in core and "R_T0_MASK=(1u<<R_T0_BITS)-1u" in core
    eng = re.sub(r"\s+", "", _src("sfl_engine.h"))
    assert 'if(t_hi>8191||ed_min-2<-8192)returnno("%s");' % lm.NOTE_HORIZON.replace(" ", "") in eng
    assert 'if(span>511)returnno("%s");' % lm.NOTE_SPAN.replace(" ", "") in eng
    assert (lm.T_HI_MAX, lm.SPAN_MAX) == (8191, 511)
    # the formula span_and_t_hi restates
    for rule in ("span=(int64_t)(dist_max>2*len_max+2?dist_max:2*len_max+2)+4",
                 "t_hi=(int64_t)(ed_max>md->max_episode_steps?ed_max:md->max_episode_steps)+2+span"):
        assert rule in eng, rule


def test_cases_name_one_kernel_family_each():
    got = [lm.predict(c)[0] for c in lm.EPOCH_CASES]
    assert got == [10, 6, 7, 8, 11, 2, 5, 0], got
    assert lm.predict(lm.EPOCH_HPG)[0] == 6 and sh.wave64_variant(*lm.EPOCH_PART.row[:2]) == 3
    assert [lm.predict(c, lm.horizon_key(c.row))[0] for c in lm.HORIZON_CASES] == [6, 8, 3]
    assert [lm.predict(lm.Case(None, g, None), lm.span_key(lm.SPAN_ON))[0] for g in lm.SPAN_GS] == [10, 1]
    assert [lm.predict(c)[0] for c in lm.DRAW_CASES] == [6, 11, 1, 10, 3, 3, 4, 4]
    assert sorted(sh.predict(c)[0] for c in lm.NO_TABLE_CASES) == [2, 5, 7, 10, 11] and len(lm.NO_TABLE_DRAW) == 2


# ---- A. the epoch wrap: host build == oracle ---------------------------------------------------------------------
def _envs(row):
    """The envs the GPU cases of a row compare with the oracle: the first, and the last of each batch size."""
    cases = lm.EPOCH_CASES + (lm.EPOCH_HPG, lm.EPOCH_PART)
    return sorted({0} | {sh.n_envs(c.G) - 1 for c in cases if c.row == row})


@pytest.mark.slow
@pytest.mark.parametrize("row", lm.EPOCH_ROWS, ids=lambda r: "%dx%dk%d" % r[:3])
def test_epoch_wrap_host_build_equals_oracle(row):
    """learn(600, exploit_freq=50) and sfl_step chunks (2044, 2200) at max_steps = 7: the oracle resets at least 520
    times in each, so the host build's slot epoch wraps at resets 256 and 511; the first chunk ends inside the episode
    the first wrap begins.  The host build's learn outputs and Q dict equal the oracle's in the envs the GPU cases
    compare."""
    envs = _envs(row)
    n = envs[-1] + 1
    out, _ = lm.epoch_host_learn(row, n)
    b = runtime.Batch(sh.compiled(row), sh.HP, sh.seeds(n), lib=hostsim.lib(), ntab=sh.NTAB, max_steps=lm.EPOCH_MAX_STEPS)
    again = b.learn(**lm.EPOCH_LEARN)  # (the cached run again, for its Q dicts)
    assert all(np.array_equal(again[k], out[k]) for k in sh.LEARN_KEYS)
    for e in envs:
        ref = lm.epoch_oracle_learn(row, sh.seeds(n)[e])
        assert ref["resets"] >= lm.EPOCH_RESETS > lm.WRAPS[1]
        assert not lm.epoch_learn_mismatches(out, e, ref), f"env {e}"
        assert b.q_dict(e) == ref["q"], f"env {e}"
    b.close()
    b = sh.stepped(sh.compiled(row), sh.HP, sh.seeds(n), hostsim.lib(), lm.EPOCH_CHUNKS, max_steps=lm.EPOCH_MAX_STEPS)
    for e in envs:
        q, at = lm.epoch_oracle_plain(row, sh.seeds(n)[e])
        assert len(at) >= lm.EPOCH_RESETS
        assert at[lm.WRAPS[0] - 1] < lm.EPOCH_CHUNKS[0] < at[lm.WRAPS[0]]  # the chunk boundary is inside that episode
        assert b.q_dict(e) == q, f"env {e}"
    b.close()


@pytest.mark.slow
def test_epoch_wrap_grouped_host_build_equals_oracle():
    """The hyperparameter-group case's reference: every grouped env the GPU case samples equals the oracle run with
    its group's hyperparameters."""
    row, n = lm.EPOCH_HPG.row, sh.n_envs(lm.EPOCH_HPG.G)
    b = sh.stepped(sh.compiled(row), sh.HANDLE_HP, sh.hpg_seeds(n), hostsim.lib(), lm.EPOCH_CHUNKS,
                   hparam_groups=sh.GROUPS, env_group=sh.env_groups(n), max_steps=lm.EPOCH_MAX_STEPS)
    for e in (n - 2, n - 1):
        q, at = lm.epoch_oracle_plain(row, sh.hpg_seeds(n)[e], e % 2)
        assert len(at) >= lm.EPOCH_RESETS and b.q_dict(e) == q, f"env {e}"
    b.close()


# ---- B. the semaphore record on and one past its limits ---------------------------------------------------------------
@pytest.mark.parametrize("row", sorted({c.row for c in lm.HORIZON_CASES}), ids=lambda r: "%dx%d" % r[:2])
def test_horizon_scenarios_sit_on_and_one_past_the_limit(row):
    for over, want in ((0, lm.T_HI_MAX), (1, lm.T_HI_MAX + 1)):
        key = lm.horizon_key(row, over)
        sc, cm = sh.scenario(key), sh.compiled(key)
        span, t_hi = lm.span_and_t_hi(cm, sc)
        late = [t.earliest_departure for t in sc.trains[::3]]
        print(f"{row[:2]} over {over}: span {span}, t_hi {t_hi}, max_episode_steps {sc.max_episode_steps}, "
              f"late departures {min(late)}..{max(late)}")
        assert t_hi == want and span <= lm.SPAN_MAX
        assert len(late) >= len(sc.trains) // 3 and min(late) >= sc.max_episode_steps - 100 - 61
        assert max(late) == sc.max_episode_steps - lm.LATE


def test_span_scenarios_sit_under_and_one_past_the_limit():
    got = []
    for spacing in (lm.SPAN_ON, lm.SPAN_PAST):
        key = lm.span_key(spacing)
        got.append(lm.span_and_t_hi(sh.compiled(key), sh.scenario(key)))
    assert [g[0] for g in got] == [508, 512] and max(g[1] for g in got) <= lm.T_HI_MAX, got


@pytest.mark.slow
@pytest.mark.parametrize("case", lm.HORIZON_CASES, ids=lm.case_id)
def test_horizon_host_build_equals_oracle(case):
    """The learn the GPU cases run on the t_hi = 8191 map: the host build's last env equals the oracle; and the step
    run's second snapshot stands past tick 8000 with a record whose start tick needs the 14-bit field's top bit."""
    key, n = lm.horizon_key(case.row), sh.n_envs(case.G)
    learn = lm.HORIZON_LEARN[case.row[:2]]
    out, _ = sh.host_learn(key, 100_000, n, **learn)
    assert out["ticks"].max() == sh.scenario(key).max_episode_steps
    ref = sh.oracle_learn(key, sh.seeds(n)[n - 1], 100_000, False, **learn)
    assert not sh.learn_mismatches(out, n - 1, ref, **learn)
    b = runtime.Batch(sh.compiled(key), sh.HP, sh.seeds(n), lib=hostsim.lib(), ntab=sh.NTAB)
    b.learn(**learn)
    assert b.q_dict(n - 1) == ref["q"]
    b.close()
    assert _late_envs(key, n, lm.HORIZON_CHUNKS[case.row[:2]])


def _late_envs(key, n, chunks):
    """Envs of the host build's second snapshot that stand past tick 8000 and hold a present record with t0 >= 4096."""
    snaps, seen = lm.host_stepped_snapshots(key, chunks, n)
    late = []
    for e, s in enumerate(snaps[1]):
        present, t0, _ = lm.sem_fields(s[2][2])
        if s[2][0] > 8000 and (t0[present] >= 4096).any():
            late.append(e)
    print(f"{key}: envs past tick 8000 with a record of t0 >= 4096: {late}; largest t0 {max(x[1] for x in seen)}")
    return late


def test_span_host_build_equals_oracle():
    """sfl_step chunks (100, 200) on the span-508 map: the host build's last envs equal the oracle, and records of a
    duration beyond 255 ticks -- the 9-bit field's top bit -- are present at both snapshots."""
    key = lm.span_key(lm.SPAN_ON)
    n = sh.n_envs(min(lm.SPAN_GS))
    snaps, seen = lm.host_stepped_snapshots(key, lm.SPAN_CHUNKS, n)
    print("largest (duration, t0) at each snapshot:", seen)
    assert all(255 < d <= lm.SPAN_MAX for d, _ in seen)
    b = sh.stepped(sh.compiled(key), sh.HP, sh.seeds(n), hostsim.lib(), lm.SPAN_CHUNKS)
    for g in lm.SPAN_GS:
        e = sh.n_envs(g) - 1
        assert b.q_dict(e) == lm.oracle_stepped(key, sh.seeds(n)[e], sum(lm.SPAN_CHUNKS))[0], f"env {e}"
    b.close()


# ---- C. the rejected exploratory draw ------------------------------------------------------------------------------
def _self_test(value, n, bound):
    f = hostsim.lib().dll.sflh_rng_selftest
    P = C.POINTER
    f.argtypes = [C.c_uint32, C.c_uint32, P(C.c_uint64), P(C.c_uint32), P(C.c_double), C.c_uint32, P(C.c_uint32)]
    o64, o32, od, ob = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n), np.zeros(n, np.uint32)
    f(value, n, o64.ctypes.data_as(P(C.c_uint64)), o32.ctypes.data_as(P(C.c_uint32)), od.ctypes.data_as(P(C.c_double)),
      bound, ob.ctypes.data_as(P(C.c_uint32)))
    return o32, ob


@pytest.mark.parametrize("v", lm.REJECTING)
def test_rejecting_sub_seeds(v):
    """scripts/lemire_rejects.cpp, a scan of all 2^31 - 1 sub-seeds with csrc/sfl_rng.h on the host, prints
        n = 2: threshold 0, no sub-seed rejects
        n = 3: threshold 1, 2 sub-seeds reject: 448450445 (pick 2) 838496653 (pick 2)
        n = 4: threshold 0, no sub-seed rejects
    For both, sfl_rng.h's first 32-bit output is 0 and its bounded draw in [0, 2] gives 2, as numpy's do; a kernel
    that skipped the rejection would pick index 0."""
    o32, ob = _self_test(v, 4, 2)
    g = np.random.default_rng(v)
    assert o32.tolist() == [int(g.integers(0, 2 ** 32)) for _ in range(4)] and o32[0] == 0
    g = np.random.default_rng(v)
    assert ob.tolist() == [int(g.integers(0, 3)) for _ in range(4)] and ob[0] == 2
    assert (0 * 3) >> 32 == 0  # the pick without the rejection
    for n in (2, 4):  # no rejection with 2 or 4 allowed actions: the threshold (2^32 - n) % n is 0
        assert (2 ** 32 - n) % n == 0
    assert (2 ** 32 - 3) % 3 == 1


@pytest.mark.parametrize("v", lm.SUB_SEEDS)
def test_crafted_state_yields_the_sub_seed(v):
    for seed in sh.seeds(3):
        words = lm.crafted_state(seed, v)
        g, plain = lm.numpy_generator(words), np.random.default_rng(seed)
        assert g.random() == plain.random()  # random() does not touch the buffered word
        assert int(g.integers(0, np.iinfo(np.int32).max)) == v
        assert g.random() == plain.random()  # and the stream goes on as the seed's
    assert [lm.crafted_buffer(x) for x in lm.REJECTING] == [1676993307, 896900891]


@pytest.mark.parametrize("row", lm.DRAW_ROWS, ids=lambda r: "%dx%d" % r[:2])
def test_draw_host_build_equals_oracle(row):
    """Given the crafted states, the oracle's first decision takes the allowed action numpy's integers(0, n) picks; in
    the two envs of the rejecting sub-seeds (seeds 300 and 301) it has three allowed actions and takes the third.  The
    host build's tables after step(20) equal the oracle's for one env of every sub-seed."""
    n = len(lm.SUB_SEEDS)
    b = runtime.Batch(sh.compiled(row), lm.HP_EXPLORE, sh.seeds(n), lib=hostsim.lib(), ntab=sh.NTAB)
    lm.draw_run(b, lm.draw_states(sh.seeds(n)))
    for e, v in enumerate(lm.SUB_SEEDS):
        ref = lm.oracle_draw(row, sh.seeds(n)[e], v)
        allowed = np.nonzero(ref["mask"])[0]
        assert ref["action"] == allowed[int(np.random.default_rng(v).integers(0, len(allowed)))]
        if v in lm.REJECTING:
            assert len(allowed) == 3 and ref["action"] == allowed[2]
        assert b.q_dict(e) == ref["q"], f"env {e}"
    b.close()


def test_draw_grouped_host_build_equals_oracle():
    row, n = lm.DRAW_HPG.row, sh.n_envs(lm.DRAW_HPG.G)
    b = runtime.Batch(sh.compiled(row), sh.HANDLE_HP, sh.seeds(n), lib=hostsim.lib(), ntab=sh.NTAB,
                      hparam_groups=lm.GROUPS_EXPLORE, env_group=sh.env_groups(n))
    lm.draw_run(b, lm.draw_states(sh.seeds(n)))
    for e in (0, 1):
        ref = lm.oracle_draw(row, sh.seeds(n)[e], lm.SUB_SEEDS[e], e % 2)
        assert ref["action"] == np.nonzero(ref["mask"])[0][2] and b.q_dict(e) == ref["q"], f"env {e}"
    assert all(not sh.same_env(x, y) for x, y in zip(sh.snapshot(b, n), lm.host_draw(row, n, True)))
    b.close()


def test_scan_program_is_committed():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "lemire_rejects.cpp")
    src = open(path).read()
    assert '#include "sfl_rng.h"' in src and all(str(v) in src for v in lm.REJECTING)
