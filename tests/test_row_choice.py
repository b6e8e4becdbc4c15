"""Seeded adversarial Q-tables (tests/_qfuzz.py) without a GPU: the host build of the lane body (sfl_core.h row_max /
max_action) against the oracle on the loaded tables, bit for bit, and the proof that each case hits what it is meant
for -- counted on the oracle alone (qf.instrument), asserted here, so that tests/test_row_choice_gpu.py, which reuses
the same inputs, compares the wave kernels on decisions of those kinds."""
import numpy as np
import pytest

from tests import _qfuzz as qf
from tests import _shapes as sh

KEYS = list(dict.fromkeys((c.cell.row, c.profile, c.hp) for c in qf.CASES))


def _id(key):
    row, profile, hp = key
    return "%sx%sk%s-%s-%s" % (row[-4], row[-3], row[-2], profile, hp)


def _slow(key):
    return [pytest.mark.slow] if key[0][-4] == 257 else []


def targets(row, profile, hp):
    """Lower bounds on the oracle's hit counts (summed over the case's oracle envs) a case is meant to reach:
    (i) forbidden and (ii) filler_wins wherever decisions are greedy and STOP does not always win; (iii) a tie of a
    stored column with a lower filler for the tie profiles, with a higher filler (the in-port's routes are the
    switch's first actions: in-port 0 only) where every decision is greedy; (iv) stale on the one-station maps;
    (v) a truncated episode for stop_high."""
    t = {}
    if hp != "eps1" and profile != "stop_high":
        t.update(forbidden=3, filler_wins=3)
    if hp != "eps1" and profile in ("ties", "zeros"):
        t.update(tie_filler_low=3)
        if hp in ("eps0", "hpg"):
            t.update(tie_filler_high=3)
    if row[0] == "one-station":
        t.update(stale=3)
    if profile == "stop_high":
        t.update(truncated=1)
    return t


def test_cells_name_the_kernels_they_claim():
    assert {c.name: qf.predict(c) for c in qf.CELLS} == qf.EXPECT
    by = {}
    for c in qf.CASES:
        by.setdefault(c.cell.name, set()).add((c.profile, c.hp))
    for name in qf.FULL:  # every profile on the G = 16, G = 64 ring and k_run cells
        assert {p for p, _ in by[name]} == set(qf.PROFILES)
    for c in qf.CELLS:    # ties and eps = 0 on every cell
        assert ("ties", "hpg" if c.hpg else "eps0") in by[c.name]
    assert {sh.VARIANTS[v][3] for v, _ in qf.EXPECT.values() if v} == {8, 16, 32, 64}


def test_tables_keep_the_layout_invariants():
    cm = sh.compiled(qf.CELLS[0].row)
    for profile in qf.PROFILES:
        dq = qf.hparams(profile, "eps0")["default_q"]
        q, t = qf.table(cm, profile, dq, 3)
        q2, t2 = qf.table(cm, profile, dq, 3)
        assert np.array_equal(q.view(np.uint64), q2.view(np.uint64)) and np.array_equal(t, t2)  # seeded
        bits = np.unpackbits(t.view(np.uint8), bitorder="little")[:cm.rows_per_env].astype(bool)
        assert abs(bits.mean() - qf.TOUCH_P[profile]) < 0.02
        A = cm.arrays
        for s in range(cm.S):
            for slot in range(len(cm.ports[s])):
                g = 4 * s + slot
                n, w = (1 << len(cm.ports[s])) * cm.K * 3, int(A["q_w"][g])
                rows = q[int(A["q_off"][g]): int(A["q_off"][g]) + n * w].reshape(n, w)
                on = bits[int(A["row_base"][g]): int(A["row_base"][g]) + n]
                assert (rows[~on] == dq).all()  # an untouched row is default_q in every column
                if profile == "stop_high":
                    assert (rows[:, w - 1] == dq + 1000.0).all()
        assert np.isfinite(q).all()
    assert np.array_equal(np.array(qf.ZERO_SET).view(np.uint64),
                          np.array([0, 1 << 63, 1, (1 << 63) | 1, 1 << 52], np.uint64))


def test_bit_comparisons_tell_the_zeros_apart():
    a, b = np.array([0.0, 1.5]), np.array([-0.0, 1.5])
    assert np.array_equal(a, b) and not qf.same_bits(a, b) and qf.same_bits(a, a.copy())
    assert qf.same_bits(np.arange(3, dtype=np.int32), np.arange(3, dtype=np.int32))
    env = (0, 0, np.zeros(2, np.uint64), np.zeros(1, np.int32), np.zeros(1, np.uint32))
    t = np.zeros(1, np.uint32)
    assert qf.same_env_bits((a, t, env), (b, t, env)) == ["Q-table bits"] and not sh.same_env((a, t, env), (b, t, env))
    assert not qf.same_env_bits((a, t, env), (a.copy(), t, env))
    assert qf.dict_bits({(1,): [0.0]}) != qf.dict_bits({(1,): [-0.0]})


@pytest.mark.parametrize("key", [pytest.param(k, id=_id(k), marks=_slow(k)) for k in KEYS])
def test_host_build_equals_oracle(key):
    """The host build's Q dict after the run (and test(1)'s outputs for the greedy driver) equal the oracle's on the
    same loaded table, as bit patterns, in the case's oracle envs; and the oracle reached the case's targets."""
    row, profile, hp = key
    _, out, _ = qf.host(row, profile, hp)
    loaded, after = qf.q_dicts(row, profile, hp)
    total = dict.fromkeys(qf.HITS, 0)
    for e in qf.oracle_envs(row, hp == "hpg"):
        q, oout, hits = qf.oracle(row, profile, hp, e)
        assert len(loaded[e]) > 0
        assert qf.dict_bits(after[e]) == qf.dict_bits(q), f"env {e}: Q dict"
        if oout is not None:
            got = (int(out["arrived"][0, e]), out["delays"][0, :, e].astype(float).tolist())
            assert got == (oout[1], [float(x) for x in oout[2]]), f"env {e}: test outputs"
            assert qf.same_bits(out["cum_reward"][0, e:e + 1], np.array([oout[0]], np.float64)), f"env {e}: cum_reward"
        for k in hits:
            total[k] += hits[k]
    print("hits", _id(key), total)
    want = targets(row, profile, hp)
    assert all(total[k] >= v for k, v in want.items()), (total, want)
