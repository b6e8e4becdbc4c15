"""Episodes recorded on the device (runtime.EvalBatch.record / recording / traffic; include/sfl.h sfl_bank_record states
the rule): the shared cases of tests/test_record.py (host build) and tests/test_record_gpu.py (MI355X).

The reference is the Python oracle: ``oracle_episode`` runs one greedy episode of one env (``sfl_oracle.build`` with
``trace=True`` for the D / S events of every decision, the table as ``model.q``, ``rail_env.step`` wrapped -- as
tests/_diag.py does -- to record every train's state, position, direction and malfunction counter after every tick).
Everything is an integer and compared exactly.  Maps, tables and seeds are the bank tests' own (tests/_evalbank.py)."""
import functools
from collections import namedtuple

import numpy as np

from oracle import sfl_oracle as so
from tests import _evalbank as eb
from tests import _qfuzz as qf
from tests import _shapes as sh

runtime = sh.runtime
parity = sh.parity
_lib = eb._lib

S_MALF, S_DONE = 5, 6
FRAME_KEYS = ("cell", "heading", "state", "malfunction")

# cell / heading / state / malfunction [n][T] after each of the n ticks (heading -1 off the map); rows: per decision
# (now, agent name, train, obs tuple, reward, mask list, action, next_switch (r, c), step_now)
OEpisode = namedtuple("OEpisode", "n cell heading state malfunction rows truncated")


@functools.lru_cache(maxsize=None)
def oracle_episode(rw, seed, table, max_steps):
    """One greedy episode of ``seed`` on table ``table`` (0: (a), 1: (b), 2: (c) of _evalbank.tables) of the row's map."""
    cm = sh.compiled(rw)
    q = runtime.raw_to_dict(cm, sh.HP["default_q"], *eb.tables(rw)[table])
    env, model = so.build(sh.scenario(rw), seed, sh.HP, max_steps=max_steps, trace=True)
    model.q = {tuple(k): list(v) for k, v in q.items()}
    ticks = []
    orig = env.rail_env.step

    def step(actions):
        r = orig(actions)
        ticks.append([(int(a.state), a.position, a.direction, int(a.malfunction_handler.malfunction_down_counter))
                      for a in env.rail_env.agents])
        return r
    env.rail_env.step = step
    model.test()
    assert ticks and len(ticks) == env.rail_env._elapsed_steps
    W = cm.W
    cell = np.array([[p[0] * W + p[1] if p is not None else -1 for _, p, _, _ in tk] for tk in ticks], np.int32)
    heading = np.array([[int(d) if p is not None else -1 for _, p, d, _ in tk] for tk in ticks], np.int32)
    state = np.array([[s for s, _, _, _ in tk] for tk in ticks], np.uint8)
    malf = np.array([[m for _, _, _, m in tk] for tk in ticks], np.int32)
    rows, ev = [], model.events
    for i, e in enumerate(ev):
        if e[0] == "D" and i + 1 < len(ev) and ev[i + 1][0] == "S":
            _, now, name, train, obs, rew, mask, _, _ = e
            _, action, nxt, _, step_now, _ = ev[i + 1]
            rows.append((now, name, train, tuple(obs), int(rew), list(mask), action, tuple(nxt), step_now))
    return OEpisode(len(ticks), cell, heading, state, malf, rows, bool(env.truncated))


def row_of(cm, ep, d):
    """Decision d of a recorded episode in the oracle's form."""
    dec = ep.decisions
    s = int(dec["switch"][d])
    na = int(cm.n_actions[s])
    return (int(dec["now"][d]), dec["agent"][d], int(dec["train"][d]), tuple(dec["obs"][d]), int(dec["reward"][d]),
            [(int(dec["mask"][d]) >> a) & 1 for a in range(na)], int(dec["action"][d]),
            tuple(cm.switch_ids[int(dec["next_switch"][d])]), int(dec["step_now"][d]))


def oracle_mismatches(cm, ep, o, tick_cap=None, dec_cap=None):
    """What of a recorded episode differs from the oracle's: the counts, every kept frame (heading on the map only) and
    every kept decision row."""
    bad = []
    if ep.ticks != o.n or ep.n_decisions != len(o.rows):
        bad.append(f"counts {ep.ticks, ep.n_decisions} != {o.n, len(o.rows)}")
    nf = o.n if tick_cap is None else min(o.n, tick_cap)
    nr = len(o.rows) if dec_cap is None else min(len(o.rows), dec_cap)
    if ep.frames != nf or ep.rows != nr:
        return bad + [f"kept {ep.frames, ep.rows} != {nf, nr}"]
    if not (ep.cell.dtype == np.int32 and np.array_equal(ep.cell, o.cell[:nf])):
        bad.append("cell")
    if not np.array_equal(ep.state, o.state[:nf]):
        bad.append("state")
    on = o.cell[:nf] >= 0
    if not np.array_equal(ep.heading[on], o.heading[:nf][on]):
        bad.append("heading")
    if not np.array_equal(ep.malfunction.astype(np.int32), o.malfunction[:nf]):
        bad.append("malfunction")
    for d in range(nr):
        if row_of(cm, ep, d) != o.rows[d]:
            bad.append(f"row {d}: {row_of(cm, ep, d)} != {o.rows[d]}")
            break
    return bad


def episode_mismatches(a, b):
    """What of two recorded episodes differs (device against host build): everything."""
    bad = [k for k in ("env", "seed", "policy", "ticks", "n_decisions", "tick_cap", "dec_cap") if getattr(a, k) != getattr(b, k)]
    bad += [k for k in FRAME_KEYS if not (getattr(a, k).dtype == getattr(b, k).dtype and np.array_equal(getattr(a, k), getattr(b, k)))]
    bad += [k for k in _lib.REC_DEC_FIELDS if not np.array_equal(a.decisions[k], b.decisions[k])]
    bad += [k for k in ("obs", "agent") if a.decisions[k] != b.decisions[k]]
    return bad


def restate_traffic(cm, episodes):
    """sfl_bank_record_traffic in numpy from recorded episodes."""
    HW = cm.H * cm.W
    out = {k: np.zeros(HW if i < 3 else cm.S, np.uint32) for i, k in enumerate(_lib.TRAFFIC_FIELDS)}
    for ep in episodes:
        c = ep.cell.astype(np.int64)
        on = c >= 0
        np.add.at(out["occupancy"], c[on], 1)
        stand = np.zeros_like(on)
        stand[1:] = on[1:] & (c[1:] == c[:-1])
        np.add.at(out["standing"], c[stand], 1)
        sm = stand & (ep.state == S_MALF)
        np.add.at(out["standing_malfunction"], c[sm], 1)
        sw = ep.decisions["switch"].astype(np.int64)
        np.add.at(out["decisions"], sw, 1)
        stop = ep.decisions["action"] == cm.n_actions[sw] - 1
        np.add.at(out["stops"], sw[stop], 1)
    for k in _lib.TRAFFIC_FIELDS[:3]:
        out[k] = out[k].reshape(cm.H, cm.W)
    return out


def traffic_mismatches(got, want):
    return [k for k in _lib.TRAFFIC_FIELDS if not (got[k].dtype == np.uint32 and got[k].shape == want[k].shape and
                                                   np.array_equal(got[k], want[k]))]


def policy_of(n, kind):
    return tuple(1 for _ in range(n)) if kind == "b" else eb.assign(n, kind)


def recorded(lib, rw, n, max_steps, kind, envs, n_policies=eb.P, **caps):
    """(EvalBatch, policy, evaluate()'s outputs) of n envs on assignment ``kind`` with ``envs`` recorded."""
    pol = policy_of(n, kind)
    ev = eb.bank(lib, rw, n, max_steps, n_policies)
    try:
        ev.record(envs, **caps)
        return ev, pol, ev.evaluate(pol)
    except BaseException:
        ev.close()
        raise


def check_against_oracle(ev, out, rw, pol, max_steps, envs, slots, **caps):
    """Slots ``slots`` (of the recorded list ``envs``) against the oracle; returns the oracle's episodes by slot."""
    cm = sh.compiled(rw)
    seeds = qf.seeds(ev.E)
    os_ = {}
    for k in slots:
        e = envs[k]
        o = os_[k] = oracle_episode(rw, seeds[e], pol[e], max_steps)
        ep = ev.recording(k)
        assert (ep.env, ep.seed, ep.policy) == (e, seeds[e], pol[e])
        assert ep.ticks == int(out["ticks"][e]) and ep.n_decisions == int(out["decisions"][e])
        bad = oracle_mismatches(cm, ep, o, caps.get("max_ticks"), caps.get("max_decisions"))
        assert not bad, (k, e, bad[:4])
    return os_


def run_device_case(lib, rw, n, max_steps, kind, envs=None, expect=None, traffic=True, **caps):
    """A device handle beside a host-build handle on the same evaluation with ``envs`` (default: all) recorded: every
    recorded array of every slot equals the host build's, the slots of envs 0, 1, 2 and n - 1 equal the oracle's, the
    evaluation's outputs are the host build's, and the traffic fold of every policy equals the host build's and the
    numpy restatement."""
    from tests import hostsim
    envs = list(range(n)) if envs is None else list(envs)
    host_ev, pol, host_out = recorded(hostsim.lib(), rw, n, max_steps, kind, envs, **caps)
    try:
        ev, _, out = recorded(lib, rw, n, max_steps, kind, envs, **caps)
        try:
            if expect is not None:
                c = ev.counters()
                assert (c["kernel_variant"], c["group_lanes"]) == expect, c
            assert all(qf.same_bits(out[k], host_out[k]) for k in eb.OUT_KEYS + ("truncated", "at_dest"))
            eps = [ev.recording(k) for k in range(len(envs))]
            for k, ep in enumerate(eps):
                bad = episode_mismatches(ep, host_ev.recording(k))
                assert not bad, (k, envs[k], bad)
            slots = [k for k, e in enumerate(envs) if e in (0, 1, 2, n - 1)]
            check_against_oracle(ev, out, rw, pol, max_steps, envs, slots, **caps)
            if traffic:
                cm = sh.compiled(rw)
                for p in range(ev.P):
                    got = ev.traffic(p)
                    assert not traffic_mismatches(got, host_ev.traffic(p)), p
                    assert not traffic_mismatches(got, restate_traffic(cm, [ep for ep in eps if ep.policy == p])), p
                last, total = ev.record_ms()
                assert 0.0 < last <= total
            return eps
        finally:
            ev.close()
    finally:
        host_ev.close()
