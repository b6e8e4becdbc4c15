"""The non-arrival diagnosis of policy-bank evaluation (runtime.EvalBatch.diagnose; include/sfl.h sfl_bank_diag states
the rule): the shared cases of tests/test_eval_diag.py (host build) and tests/test_eval_diag_gpu.py (MI355X).

The reference is the Python oracle: ``oracle_episode`` runs one greedy episode of one env as
scripts/diagnose_nonarrivals.py's ``greedy_episode`` does (``sfl_oracle.build``, the table as ``model.q``,
``rail_env.step`` wrapped to record every train's state, position and direction per tick, ``model.test()``), and
``classify`` restates the rule on those records with the oracle's own ``action_valid`` / ``check_action_on_agent``.
Everything is an integer and compared exactly.  Maps, tables and seeds are the bank tests' own (tests/_evalbank.py)."""
import functools
from collections import namedtuple

import numpy as np

from oracle import flatland_lite as fl
from oracle import sfl_oracle as so
from tests import _evalbank as eb
from tests import _qfuzz as qf
from tests import _shapes as sh

runtime = sh.runtime
parity = sh.parity
_lib = eb._lib

ARRIVED, TRUNCATED, NEVER_DEPARTED, MOVING_LATE, STOP_LOOP, DEADLOCK_QUEUE, DEADLOCK_CYCLE = range(7)
ACTIONS = (fl.RailEnvActions.MOVE_FORWARD, fl.RailEnvActions.MOVE_LEFT, fl.RailEnvActions.MOVE_RIGHT)

# n ticks; truncated; pos [n + 1][T] tuples or None (row 0: before the first tick, every train off the map); the final
# state and direction per train; the rail
Episode = namedtuple("Episode", "n truncated pos state direction rail")
# [T] arrays of one env, cells as r * W + c (-1: off the map), and the trains' final MALFUNCTION flags
Diag = namedtuple("Diag", "cls blocker stalled_for cell stalled malf")


@functools.lru_cache(maxsize=None)
def oracle_episode(rw, seed, table, max_steps):
    """One greedy episode of ``seed`` on table ``table`` (0: (a), 1: (b), 2: (c) of _evalbank.tables) of the row's map."""
    cm = sh.compiled(rw)
    q = runtime.raw_to_dict(cm, sh.HP["default_q"], *eb.tables(rw)[table])
    env, model = so.build(sh.scenario(rw), seed, sh.HP, max_steps=max_steps, trace=False)
    model.q = {tuple(k): list(v) for k, v in q.items()}
    ticks = []
    orig = env.rail_env.step

    def step(actions):
        r = orig(actions)
        ticks.append([(a.state, a.position, a.direction) for a in env.rail_env.agents])
        return r
    env.rail_env.step = step
    model.test()
    T = len(env.rail_env.agents)
    assert ticks and len(ticks) == env.rail_env._elapsed_steps
    pos = [[None] * T] + [[tuple(p) if p is not None else None for _, p, _ in tk] for tk in ticks]
    return Episode(len(ticks), bool(env.truncated), pos, [s for s, _, _ in ticks[-1]], [d for _, _, d in ticks[-1]],
                   env.rail_env.rail)


def classify(ep, stall, W):
    """The rule of include/sfl.h on an oracle episode."""
    T, n = len(ep.state), ep.n
    last = ep.pos[n]
    L = [max([i for i in range(1, n + 1) if ep.pos[i][h] != ep.pos[i - 1][h]], default=0) for h in range(T)]
    sf = [n - L[h] if last[h] is not None else -1 for h in range(T)]
    stalled = [last[h] is not None and sf[h] >= min(stall, n) - 1 for h in range(T)]
    for h in range(T):  # (the script's statement of the same: the last `stall` recorded positions equal the final one)
        window = [ep.pos[i][h] for i in range(1, n + 1)][-stall:]
        assert stalled[h] == (last[h] is not None and all(p == last[h] for p in window)), (h, stall)
    held = {}
    for h in range(T):
        if last[h] is not None:
            held[last[h]] = h
    blocker = [-1] * T
    for h in range(T):
        if not stalled[h]:
            continue
        for act in ACTIONS:
            if fl.action_valid(ep.rail, act, last[h], ep.direction[h]):
                _, (p2, _), _, _ = ep.rail.check_action_on_agent(act, (last[h], ep.direction[h]))
                j = held.get(tuple(p2))
                if j is not None and stalled[j]:
                    blocker[h] = j
                    break
    cls = []
    for h in range(T):
        x, on_cycle = blocker[h], False
        for _ in range(T):
            if x < 0:
                break
            if x == h:
                on_cycle = True
                break
            x = blocker[x]
        if ep.state[h] == fl.TrainState.DONE:
            c = ARRIVED
        elif ep.truncated:
            c = TRUNCATED
        elif last[h] is None:
            c = NEVER_DEPARTED
        elif not stalled[h]:
            c = MOVING_LATE
        elif blocker[h] < 0:
            c = STOP_LOOP
        else:
            c = DEADLOCK_CYCLE if on_cycle else DEADLOCK_QUEUE
        cls.append(c)
    cell = [p[0] * W + p[1] if p is not None else -1 for p in last]
    malf = [ep.state[h] == fl.TrainState.MALFUNCTION for h in range(T)]
    return Diag(np.array(cls, np.uint8), np.array(blocker, np.int16), np.array(sf, np.int32), np.array(cell, np.int32),
                np.array(stalled), np.array(malf))


def oracle_diag(rw, seed, table, max_steps, stall):
    return classify(oracle_episode(rw, seed, table, max_steps), stall, sh.compiled(rw).W)


def oracle_counts(diags):
    """Class value -> trains, over some envs' oracle diagnoses."""
    return np.bincount(np.concatenate([d.cls for d in diags]), minlength=7)


def cycle_members(diags):
    return int(sum((d.cls == DEADLOCK_CYCLE).sum() for d in diags))


# ---- comparisons ------------------------------------------------------------------------------------------------------------
def final_cells(ev, e):
    """Train cells [T] of env e's end state (sfl_get_env_state, either layout class)."""
    return parity.env_state(ev, e)[3]


def env_mismatches(ev, got, e, d):
    """What of env e's diagnosis (``got``: diagnose()'s per-train arrays) differs from the oracle's ``d``."""
    bad = [k for k, ref in (("cls", d.cls), ("blocker", d.blocker), ("stalled_for", d.stalled_for))
           if not (got[k][:, e].dtype == ref.dtype and np.array_equal(got[k][:, e], ref))]
    if not np.array_equal(final_cells(ev, e), d.cell):
        bad.append("cells")
    return [f"env {e}: {k}" for k in bad]


def hot_of(cm, policy, n_policies, cls, cells):
    """[P][H][W] hotspot counts from per-env (cls [T], cells [T]) pairs in env order."""
    hot = np.zeros((n_policies, cm.H * cm.W), np.uint32)
    for e, (c, cell) in enumerate(zip(cls, cells)):
        for h in np.nonzero(c >= STOP_LOOP)[0]:
            hot[policy[e], cell[h]] += 1
    return hot.reshape(n_policies, cm.H, cm.W)


def restate_cells(got, ticks, stall, policy, n_policies, malf=None):
    """sfl_diag_cell in numpy from diagnose()'s per-train arrays ([T][E]), the episodes' ticks [E] and, where known, the
    trains' final MALFUNCTION flags [T][E] (else that word is left out)."""
    cls, blk, sf = got["cls"], got["blocker"].astype(np.int64), got["stalled_for"].astype(np.int64)
    T, E = cls.shape
    policy = np.asarray(policy)
    stalled = (sf >= 0) & (sf >= np.minimum(stall, ticks.astype(np.int64))[None, :] - 1)
    cycles = np.zeros(E, np.int64)
    for e in range(E):
        for h in np.nonzero(cls[:, e] == DEADLOCK_CYCLE)[0]:
            x, lo = blk[h, e], h
            for _ in range(T):
                if x < 0 or x == h:
                    break
                lo = min(lo, x)
                x = blk[x, e]
            cycles[e] += x == h and lo == h
    cells = {k: np.zeros(n_policies, np.int64) for k in _lib.DIAG_FIELDS if k != "stalled_in_malfunction" or malf is not None}
    for p in range(n_policies):
        m = policy == p
        cells["episodes"][p] = m.sum()
        for c, k in enumerate(_lib.DIAG_CLASSES):
            if c:
                cells[k][p] = (cls[:, m] == c).sum()
        cells["cycles"][p] = cycles[m].sum()
        cells["episodes_jammed"][p] = (cls[:, m] >= DEADLOCK_QUEUE).any(axis=0).sum()
        if malf is not None:
            cells["stalled_in_malfunction"][p] = (stalled & malf)[:, m].sum()
        cells["stalled_for_sum"][p] = np.where(stalled, sf, 0)[:, m].sum()
        cells["stalled_for_max"][p] = sf[:, m][stalled[:, m]].max() if stalled[:, m].any() else np.iinfo(np.int64).min
    return cells


def table_mismatches(table, cells, T):
    bad = [f"table.{k}" for k in cells if not (table[k].dtype == np.int64 and np.array_equal(table[k], cells[k]))]
    n = cells["episodes"]
    arrived = n * T - sum(table[k] for k in _lib.DIAG_CLASSES[1:])
    if (arrived < 0).any():
        bad.append("table: the class words exceed episodes * T")
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in _lib.DIAG_CLASSES[1:]:
            want = np.where(n > 0, cells[k] / n.astype(np.float64), np.nan)
            if not np.array_equal(table[k + "_mean"], want, equal_nan=True):
                bad.append(f"table.{k}_mean")
        want = np.where(n > 0, cells["episodes_jammed"] / n.astype(np.float64), np.nan)
    if not np.array_equal(table["jammed_frac"], want, equal_nan=True):
        bad.append("table.jammed_frac")
    if not np.isnan(table["jammed_frac"][n == 0]).all() or not np.isnan(table["stop_loop_mean"][n == 0]).all():
        bad.append("table: a policy without episodes has a mean")
    return bad


def check_against_oracle(ev, got, ev_out, rw, policy, max_steps, stall, envs=None):
    """The diagnosis ``got`` of the evaluation ``ev_out`` against the oracle on ``envs`` (default: all): per-train arrays
    and cells; when every env is checked, also the table, the arrived trains and the hotspots.  Returns the oracle's
    diagnoses by env."""
    cm = sh.compiled(rw)
    seeds = qf.seeds(ev.E)
    full = envs is None
    envs = list(range(ev.E)) if full else list(envs)
    ds = {e: oracle_diag(rw, seeds[e], policy[e], max_steps, stall) for e in envs}
    bad = []
    for e in envs:
        ep = oracle_episode(rw, seeds[e], policy[e], max_steps)
        if int(ev_out["ticks"][e]) != ep.n or bool(ev_out["truncated"][e]) != ep.truncated:
            bad.append(f"env {e}: ticks / truncated")
        bad += env_mismatches(ev, got, e, ds[e])
    if full:
        malf = np.stack([ds[e].malf for e in envs], axis=1)
        cells = restate_cells(got, ev_out["ticks"], stall, policy, ev.P, malf)
        bad += table_mismatches(got["table"], cells, cm.T)
        if not np.array_equal(ev_out["at_dest"].astype(bool), got["cls"] == ARRIVED):
            bad.append("class 0 is not at_dest")
        hot = hot_of(cm, policy, ev.P, [ds[e].cls for e in envs], [ds[e].cell for e in envs])
        for p in range(ev.P):
            h = ev.hotspots(p)
            if not (h.dtype == np.uint32 and h.shape == (cm.H, cm.W) and np.array_equal(h, hot[p])):
                bad.append(f"hotspots({p})")
            t = got["table"]
            if int(h.sum()) != int(t["stop_loop"][p] + t["deadlock_queue"][p] + t["deadlock_cycle"][p]):
                bad.append(f"hotspots({p}).sum()")
    assert not bad, (stall, bad[:8])
    return ds


def check_against_host(ev, got, host_ev, host_got):
    """A device diagnosis against the host build's of the same evaluation: every array, every env's cells, the table
    and the hotspots."""
    bad = [k for k in ("cls", "blocker", "stalled_for") if not np.array_equal(got[k], host_got[k])]
    bad += [f"table.{k}" for k in _lib.DIAG_FIELDS if not np.array_equal(got["table"][k], host_got["table"][k])]
    for e in range(ev.E):
        if not np.array_equal(final_cells(ev, e), final_cells(host_ev, e)):
            bad.append(f"env {e}: cells")
    bad += [f"hotspots({p})" for p in range(ev.P) if not np.array_equal(ev.hotspots(p), host_ev.hotspots(p))]
    assert not bad, bad[:8]


def evaluated(lib, rw, n, max_steps, kind, n_policies=eb.P):
    """(EvalBatch, policy, evaluate()'s outputs) of n envs on assignment ``kind`` (_evalbank.assign; "b": table (b))."""
    pol = tuple(1 for _ in range(n)) if kind == "b" else eb.assign(n, kind)
    ev = eb.bank(lib, rw, n, max_steps, n_policies)
    try:
        return ev, pol, ev.evaluate(pol)
    except BaseException:
        ev.close()
        raise


def run_device_case(lib, rw, n, max_steps, kind, stalls, expect=None, n_policies=eb.P):
    """A device handle beside a host-build handle on the same evaluation: for each window the device's diagnosis
    equals the host build's on all n envs and the oracle's on the first three and the last env."""
    from tests import hostsim
    host_ev, pol, host_out = evaluated(hostsim.lib(), rw, n, max_steps, kind, n_policies)
    try:
        ev, _, out = evaluated(lib, rw, n, max_steps, kind, n_policies)
        try:
            if expect is not None:
                c = ev.counters()
                assert (c["kernel_variant"], c["group_lanes"]) == expect, c
            assert all(qf.same_bits(out[k], host_out[k]) for k in eb.OUT_KEYS + ("truncated", "at_dest"))
            envs = sorted({0, 1, 2, n - 1} & set(range(n)))
            for s in stalls:
                got, host_got = ev.diagnose(stall=s), host_ev.diagnose(stall=s)
                check_against_host(ev, got, host_ev, host_got)
                check_against_oracle(ev, got, out, rw, pol, max_steps, s, envs=envs)
            last, total = ev.diag_ms()
            assert 0.0 < last <= total
        finally:
            ev.close()
    finally:
        host_ev.close()
