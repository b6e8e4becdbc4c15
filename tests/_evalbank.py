"""Policy-bank evaluation (runtime.EvalBatch; include/sfl.h sfl_bank_*): the shared cases of tests/test_eval_bank.py
(host build) and tests/test_eval_bank_gpu.py (MI355X).

The reference throughout is the existing code: a twin ``runtime.Batch`` on the host build with the same map, hp, seeds
and max_steps, whose env e is given table env_policy[e] with ``set_q_raw`` and which runs ``test(1)`` (tests/_qfuzz.py's
greedy driver).  Everything is compared as bit patterns; there is no tolerance anywhere.

The bank of a map has P = 3 tables: (a) the table a one-env ``learn(30)`` with _shapes.HP and seed 900 leaves, (b)
_qfuzz's "ties" table of env 0, (c) its "distinct" table of env 1.  (b) and (c) end their episodes by truncation only,
so every case they take part in runs max_steps = _qfuzz.MAX_STEPS; the (a)-only cases run 100,000.

``at_dest`` is compared with the twin's train states: a train stands at its destination when the state field of its
``tr_bits`` word is DONE (6), which is what ``DistrQLearning.test`` saves as trains_at_dest.npz.  (Bit 21 of the word,
Flatland's ``dones``, is also set for every train when the timetable's horizon ends the episode, so it cannot tell an
arrived train from one that did not arrive.)"""
import functools
from collections import namedtuple

import numpy as np

from tests import _qfuzz as qf
from tests import _shapes as sh
from tests import hostsim

runtime = sh.runtime
parity = sh.parity
_lib = qf.runtime._lib

P = 3
LONG = 100_000
OUT_KEYS = ("cum_reward", "arrived", "num_malfunctions", "decisions", "ticks", "delays")
S_DONE = 6


def row(S, T, K=8):
    r = [r for r in sh.ROWS if r[:3] == (S, T, K)]
    assert len(r) == 1
    return r[0]


# ---- the tables ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables(rw):
    """((Q block, key set) of (a), (b), (c)) on the row's map."""
    cm = sh.compiled(rw)
    b = runtime.Batch(cm, sh.HP, [900], lib=hostsim.lib(), ntab=sh.NTAB)
    b.learn(30)
    a = b.q_raw(0)
    b.close()
    dq = sh.HP["default_q"]
    return a, qf.table(cm, "ties", dq, 0), qf.table(cm, "distinct", dq, 1)


def assign(n, kind):
    """env_policy of n envs: "a" (table (a) only), "mod" (e % 3), "perm" ((7 e + 1) % 3), "ab" (e % 2: (a) and (b))."""
    return tuple({"a": 0, "mod": e % P, "perm": (7 * e + 1) % P, "ab": e % 2}[kind] for e in range(n))


# ---- the twin ------------------------------------------------------------------------------------------------------------
Twin = namedtuple("Twin", "out states truncated")


@functools.lru_cache(maxsize=None)
def twin(rw, n, policy, max_steps, episodes=1):
    """The twin's test(episodes) outputs ([episode][...][env]), every env's end state, and [episode][env] whether the
    episode was truncated (its decisions == max_steps + 1)."""
    tb = tables(rw)
    b = runtime.Batch(sh.compiled(rw), sh.HP, qf.seeds(n), lib=hostsim.lib(), ntab=sh.NTAB, max_steps=max_steps)
    for e in range(n):
        b.set_q_raw(e, *tb[policy[e]])
    out = b.test(episodes)
    states = [parity.env_state(b, e) for e in range(n)]
    b.close()
    return Twin(out, states, (out["decisions"] == max_steps + 1).astype(np.int32))


def twin_at_dest(t):
    """[T][E] from the twin's end state (valid for the last episode it ran)."""
    return np.stack([((st[4] >> 2) & 7) == S_DONE for st in t.states], axis=1).astype(np.uint8)


def restate(out, at_dest, truncated, policy, n_policies, T):
    """The fold's rule (include/sfl.h sfl_eval_cell) in numpy, from one episode's per-env arrays ([E], [T][E])."""
    policy = np.asarray(policy)
    delays, at = out["delays"].astype(np.int64), at_dest.astype(bool)
    cells = {k: np.zeros(n_policies, np.int64) for k in _lib.EVAL_FIELDS}
    for p in range(n_policies):
        m = policy == p
        c = {k: 0 for k in _lib.EVAL_FIELDS}
        c["episodes"] = int(m.sum())
        c["trains_early"] = int((at & (delays <= 0))[:, m].sum())
        c["trains_late"] = int((at & (delays > 0))[:, m].sum())
        c["trains_not_arrived"] = int((~at)[:, m].sum())
        arr, rew = out["arrived"][m].astype(np.int64), out["cum_reward"][m].astype(np.int64)
        i64 = np.iinfo(np.int64)
        c["arrived_min"], c["arrived_max"] = (int(arr.min()), int(arr.max())) if m.any() else (i64.max, i64.min)
        c["reward_min"], c["reward_max"] = (int(rew.min()), int(rew.max())) if m.any() else (i64.max, i64.min)
        c["all_arrived"] = int((arr == T).sum())
        c["reward_sum"] = int(rew.sum())
        c["decisions_sum"] = int(out["decisions"][m].astype(np.int64).sum())
        c["ticks_sum"] = int(out["ticks"][m].astype(np.int64).sum())
        c["malfunctions_sum"] = int(out["num_malfunctions"][m].astype(np.int64).sum())
        c["delay_sum_arrived"] = int(np.where(at, delays, 0)[:, m].sum())
        c["truncated"] = int(truncated[m].sum())
        for k in _lib.EVAL_FIELDS:
            cells[k][p] = c[k]
    return cells


def episode(t, i=0):
    """Episode i of a twin's outputs as per-env arrays."""
    return {k: t.out[k][i] for k in OUT_KEYS}


# ---- preconditions, asserted on the twin ---------------------------------------------------------------------------------
def envs_differ(t, policy):
    """At least two envs following the same policy differ in ticks or arrived."""
    pol = np.asarray(policy)
    return any(len({(int(a), int(b)) for a, b in zip(t.out["ticks"][0][pol == p], t.out["arrived"][0][pol == p])}) > 1
               for p in set(policy))


def classes_populated(t, policy, T):
    """Early, late and not arrived are all non-zero for at least one policy."""
    c = restate(episode(t), twin_at_dest(t), t.truncated[0], policy, P, T)
    return any(c["trains_early"][p] and c["trains_late"][p] and c["trains_not_arrived"][p] for p in range(P))


# ---- the code under test --------------------------------------------------------------------------------------------------
def bank(lib, rw, n, max_steps, n_policies=P):
    """An EvalBatch on the row's map with the row's tables set."""
    ev = runtime.EvalBatch(sh.compiled(rw), sh.HP, qf.seeds(n), n_policies, lib=lib, max_steps=max_steps)
    for p, tb in enumerate(tables(rw)[:n_policies]):
        ev.set_policy_raw(p, *tb)
    return ev


def mismatches(ev, got, t, policy, i=0, states=True):
    """What of an evaluation differs from episode i of the twin: per-env outputs, at_dest and the whole end state (those
    two for the twin's last episode only), the truncation flags, and the table against the numpy restatement of the
    fold computed from the twin's outputs."""
    T = ev.cm.T
    ref = episode(t, i)
    bad = [k for k in OUT_KEYS if not qf.same_bits(got[k], ref[k])]
    if not np.array_equal(got["truncated"], t.truncated[i]):
        bad.append("truncated")
    if not np.array_equal(got["policy"], np.asarray(policy, np.uint32)):
        bad.append("policy")
    if states:
        if not np.array_equal(got["at_dest"], twin_at_dest(t)):
            bad.append("at_dest")
        for e in range(ev.E):
            bad += [f"env {e}: {x}" for x in parity._state_diff(parity.env_state(ev, e), t.states[e])]
        cells = restate(ref, twin_at_dest(t), t.truncated[i], policy, ev.P, T)
        bad += table_mismatches(got["table"], cells, T)
    return bad


def table_mismatches(table, cells, T):
    bad = [f"table.{k}" for k in _lib.EVAL_FIELDS if not (table[k].dtype == np.int64 and np.array_equal(table[k], cells[k]))]
    n = cells["episodes"]
    if not np.array_equal(table["trains_early"] + table["trains_late"] + table["trains_not_arrived"], n * T):
        bad.append("table: early + late + not arrived != episodes * T")
    means = dict(early_mean="trains_early", late_mean="trains_late", not_arrived_mean="trains_not_arrived",
                 reward_mean="reward_sum", decisions_per_episode="decisions_sum", truncated_frac="truncated",
                 all_arrived_frac="all_arrived")
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, num in means.items():
            want = np.where(n > 0, cells[num] / n.astype(np.float64), np.nan)
            if not np.array_equal(table[k], want, equal_nan=True):
                bad.append(f"table.{k}")
        want = np.where((n > 0) & (cells["decisions_sum"] > 0), cells["ticks_sum"] / cells["decisions_sum"].astype(np.float64),
                        np.nan)
    if not np.array_equal(table["ticks_per_decision"], want, equal_nan=True):
        bad.append("table.ticks_per_decision")
    if not np.isnan(table["reward_mean"][n == 0]).all():
        bad.append("table: a policy without episodes has a mean")
    return bad


def bank_unchanged(ev, rw):
    """Case 2: every table of the bank still holds what was set, Q bits and key-set words alike."""
    bad = []
    for p, (q, t) in enumerate(tables(rw)[:ev.P]):
        gq, gt = ev.policy_raw(p)
        if not qf.same_bits(gq, q):
            bad.append(f"policy {p}: Q bits")
        if not np.array_equal(gt, t):
            bad.append(f"policy {p}: key set")
    return bad


# ---- the cases both files run ----------------------------------------------------------------------------------------------
def run_twin_equality(lib, rw, n, expect=None):
    """Cases 1 - 3 on one handle: e % 3, then the fixed permutation of it (no state of the first evaluation may leak
    into the second), each against its own twin; then the bank is unchanged.  (At max_steps = 40 few trains arrive, so
    early, late and not arrived need not all occur here: run_long asserts that precondition and runs on every cell too.)"""
    ev = bank(lib, rw, n, qf.MAX_STEPS)
    try:
        if expect is not None:
            c = ev.counters()
            assert (c["kernel_variant"], c["group_lanes"]) == expect, c
        first = True
        for kind in ("mod", "perm"):
            pol = assign(n, kind)
            t = twin(rw, n, pol, qf.MAX_STEPS)
            assert envs_differ(t, pol), "precondition (twin): envs of one policy do not differ"
            got = ev.evaluate(pol if not first else None)  # (the default assignment is e % n_policies)
            first = False
            bad = mismatches(ev, got, t, pol)
            assert not bad, f"{kind}: {bad[:8]}"
            c = ev.counters()
            assert c["last_launch_decisions"] == int(t.out["decisions"][0].sum())
            assert c["last_launch_ticks"] == int(t.out["ticks"][0].sum())
        assert not bank_unchanged(ev, rw), bank_unchanged(ev, rw)
    finally:
        ev.close()


def run_long(lib, rw, n, classes=True, expect=None):
    """Table (a) alone at max_steps = 100,000: episodes that end by termination, with early, late and not-arrived
    trains (``classes``: asserted on the twin); policies 1 and 2 have no episode."""
    T = sh.compiled(rw).T
    pol = assign(n, "a")
    t = twin(rw, n, pol, LONG)
    assert envs_differ(t, pol) and not t.truncated.any(), "precondition (twin): envs of one policy do not differ"
    assert not classes or classes_populated(t, pol, T), "precondition (twin): early, late and not arrived all populated"
    ev = bank(lib, rw, n, LONG)
    try:
        if expect is not None:
            c = ev.counters()
            assert (c["kernel_variant"], c["group_lanes"]) == expect, c
        got = ev.evaluate(pol)
        bad = mismatches(ev, got, t, pol)
        assert not bad, bad[:8]
        assert got["table"]["episodes"].tolist() == [n, 0, 0]
        assert np.isnan(got["table"]["early_mean"][1:]).all() and np.isnan(got["table"]["ticks_per_decision"][1:]).all()
        slim = ev.evaluate(pol, per_env=False)
        assert sorted(slim) == ["policy", "table"] and not table_mismatches(slim["table"], {k: got["table"][k] for k in _lib.EVAL_FIELDS}, T)
        assert not bank_unchanged(ev, rw)
    finally:
        ev.close()
    return t


def run_truncation(lib, rw, n):
    """Case 4: max_steps = 3, where every episode truncates, and max_steps = 40 with (b) beside (a)."""
    pol = assign(n, "ab")
    t3 = twin(rw, n, pol, 3)
    assert t3.truncated.all()
    t40 = twin(rw, n, pol, qf.MAX_STEPS)
    assert t40.truncated.any() and not t40.truncated.all(), "precondition (twin): truncated and untruncated episodes"
    for ms, t in ((3, t3), (qf.MAX_STEPS, t40)):
        ev = bank(lib, rw, n, ms)
        try:
            got = ev.evaluate(pol)
            bad = mismatches(ev, got, t, pol)
            assert not bad, f"max_steps {ms}: {bad[:8]}"
            assert got["table"]["truncated"].tolist() == [int(t.truncated[0][np.asarray(pol) == p].sum()) for p in range(P)]
        finally:
            ev.close()


WRAP_CALLS = 258
WRAP_CHECK = (1, 255, 256, 257, 258)


def run_epoch_wrap(lib, G=None):
    """Case 5: 258 evaluations on one handle pass the slot-epoch clear of reset 256; evaluations 1, 255, 256, 257 and 258
    equal the rows of the same index of the twin's test(258)."""
    rw = row(5, 1)
    n = sh.n_envs(G)
    pol = assign(n, "a")
    t = twin(rw, n, pol, 7, WRAP_CALLS)
    ev = bank(lib, rw, n, 7)
    try:
        for i in range(1, WRAP_CALLS + 1):
            got = ev.evaluate(pol, per_env=i in WRAP_CHECK)
            if i in WRAP_CHECK:
                bad = mismatches(ev, got, t, pol, i - 1, states=i == WRAP_CALLS)
                assert not bad, f"evaluation {i}: {bad[:8]}"
    finally:
        ev.close()


def run_copy_policy(lib, rw, n_train=6):
    """Case 6: tables copied device to device from a training batch equal q_raw / consensus_raw, and evaluate like the
    same tables uploaded from the host."""
    cm = sh.compiled(rw)
    tr = runtime.Batch(cm, sh.HP, [700 + i for i in range(n_train)], lib=lib, ntab=sh.NTAB)
    ev = ev2 = None
    try:
        tr.learn_begin()
        tr.apply_qinit()
        tr.step(50)
        tr.consensus("mean", cohorts=[e % 2 for e in range(n_train)], share=False)
        n = 12
        ev = runtime.EvalBatch(cm, sh.HP, qf.seeds(n), P, lib=lib, max_steps=qf.MAX_STEPS)
        ev.copy_policy(0, tr, env=n_train - 1)
        ev.copy_policy(1, tr, cohort=0)
        ev.copy_policy(2, tr, cohort=1)
        want = [tr.q_raw(n_train - 1), tr.consensus_raw(0), tr.consensus_raw(1)]
        for p in range(P):
            gq, gt = ev.policy_raw(p)
            assert qf.same_bits(gq, want[p][0]) and np.array_equal(gt, want[p][1]), p
        ev2 = runtime.EvalBatch(cm, sh.HP, qf.seeds(n), P, lib=lib, max_steps=qf.MAX_STEPS)
        for p in range(P):
            ev2.set_policy_raw(p, *want[p])
        a, b = ev.evaluate(), ev2.evaluate()
        for k in OUT_KEYS + ("truncated", "at_dest"):
            assert qf.same_bits(a[k], b[k]), k
        for k in _lib.EVAL_FIELDS:
            assert np.array_equal(a["table"][k], b["table"][k]), k
        assert a["table"]["episodes"].tolist() == [4, 4, 4]
        with_pytest_raises(lambda: ev.copy_policy(0, tr, cohort=2), "cohort")          # a missing cohort
        with_pytest_raises(lambda: ev.copy_policy(0, tr, env=n_train), "env")
        other = runtime.Batch(sh.compiled(row(5, 1)), sh.HP, [1], lib=lib, ntab=sh.NTAB)  # a batch of another map
        try:
            with_pytest_raises(lambda: ev.copy_policy(0, other, env=0), "layout")
        finally:
            other.close()
        a2 = ev.evaluate()  # after the refusals the handle still evaluates, and the tables are what they were
        for k in OUT_KEYS:
            assert qf.same_bits(a[k], a2[k]), k
    finally:
        for x in (tr, ev, ev2):
            if x is not None:
                x.close()


def with_pytest_raises(fn, word):
    import pytest
    with pytest.raises(_lib.SflError) as ei:
        fn()
    msg = str(ei.value)
    assert len(msg) > 10 and word in msg, msg
    return msg
