"""Suspend and resume (runtime.Batch.capture / restore / q_dicts; include/sfl.h sfl_state_*): the kernel cells, the
drivers and the checks that tests/test_state.py runs on the host build and tests/test_state_gpu.py on the MI355X.

A cell names a kernel (tests/_qfuzz.py CELLS: map row, group size, kernel-selection settings).  Every run uses
max_steps = 40 and the chunks (30, 55) of tests/_qfuzz.py: the capture after 30 decisions falls inside an episode, the
second leg crosses an episode's end and a reset.  Everything is compared as bit patterns; there is no tolerance.

The twin of a cell is the run that never stops: learn_begin, apply_qinit, step(30), step(55).  It is computed once per
(library, cell) and shared: its capture and snapshot at the capture point and at the end."""
import importlib
from types import SimpleNamespace

import numpy as np

from tests import _qfuzz as qf
from tests import _shapes as sh

runtime = sh.runtime
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")

MAX_STEPS = qf.MAX_STEPS   # 40
CHUNKS = qf.CHUNKS         # (30, 55)
SHIFT = 1000               # the seeds of a batch that is restored into differ by this much
PRE = 7                    # ... and it has itself run this many decisions
CELLS = tuple(c for c in qf.CELLS if c.name in ("g8", "g16", "v7", "g32", "g64", "ring", "krun", "hpg16"))
WAVE_CELL = "g16"          # the wave cell of the single-cell tests
KERNEL_ENV = ("SFL_KERNEL", "SFL_WAVE_G", "SFL_LDS_MAP", "SFL_REQUIRE_WAVE")
ARRAYS = tuple(name for name, _ in runtime.BatchState.ARRAYS)
Q_ARRAYS = ("touched", "row_off", "row_ids", "cell_off", "cells")   # what does not depend on the layout class
# the head of a state record, the same in both layout classes: phase, elapsed, eflags, ep_t, n_test, epoch (int32)
HEAD = dict(phase=0, elapsed=4, eflags=8, ep_t=12, n_test=16, epoch=20)


def cell(name):
    return next(c for c in CELLS if c.name == name)


def set_env(monkeypatch, c, **extra):
    """The kernel-selection settings of a cell (everything else unset)."""
    for k in KERNEL_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(qf.cell_env(c), **extra).items():
        monkeypatch.setenv(k, v)


def n_envs(c):
    return qf.n_envs(c)


def make(c, lib, n=None, shift=0, max_steps=MAX_STEPS, hp=None, **kw):
    """A batch of the cell's map: n envs (default: the cell's), seeds shifted by ``shift``."""
    n = n_envs(c) if n is None else n
    if c.hpg:
        seeds = [s + shift for s in sh.hpg_seeds(n)]
        kw = dict(dict(hparam_groups=sh.GROUPS, env_group=sh.env_groups(n)), **kw)
        hp = hp or sh.HANDLE_HP
    else:
        seeds = [s + shift for s in sh.seeds(n)]
    return runtime.Batch(sh.compiled(c.row), hp or sh.HP, seeds, lib=lib, ntab=sh.NTAB, max_steps=max_steps, **kw)


def begin(b, *chunks):
    b.learn_begin()
    b.apply_qinit()
    step(b, *chunks)
    return b


def step(b, *chunks):
    for k in chunks:
        got, _ = b.step(k)
        assert got == k * b.E
    return b


def head(state, field):
    """One int32 field of every record's head."""
    o = HEAD[field]
    return np.ascontiguousarray(state.state[:, o:o + 4]).view(np.int32).reshape(-1)


def same_state(a, b, names=ARRAYS):
    """The arrays of two captures that differ (empty: byte-identical), fingerprint and layout included."""
    bad = [k for k in names if not qf.same_bits(getattr(a, k), getattr(b, k))]
    if names is ARRAYS:
        bad += [k for k in ("fingerprint", "layout") if getattr(a, k) != getattr(b, k)]
    return bad


def section(s, k):
    """(key set, row ids, cells) of record k of a capture."""
    return (s.touched[k], s.row_ids[int(s.row_off[k]): int(s.row_off[k + 1])],
            s.cells[int(s.cell_off[k]): int(s.cell_off[k + 1])])


def mismatches(b, ref, envs=None, ref_envs=None):
    """{env: mismatching parts} of a batch's envs against snapshot entries (tests/_shapes.py same_env, Q as bits)."""
    envs = range(b.E) if envs is None else envs
    ref_envs = envs if ref_envs is None else ref_envs
    out = {}
    for e, r in zip(envs, ref_envs):
        bad = qf.same_env_bits(b.q_raw(e) + (sh.parity.env_state(b, e),), ref[r])
        if bad:
            out[e] = bad
    return out


_twins = {}


def twin(lib, c, key=""):
    """The cell's run that never stops, on ``lib`` (under the kernel settings in force at the first call; ``key`` tells
    two settings of one cell apart): mid / end captures and snapshots, the end's Q dicts through the per-env path."""
    k = (lib.path, c.name, key)
    if k not in _twins:
        n = n_envs(c)
        b = begin(make(c, lib), CHUNKS[0])
        t = SimpleNamespace(n=n, counters=b.counters(), seeds=list(b.seeds))
        t.mid, t.mid_snap = b.capture(), sh.snapshot(b, n)
        step(b, CHUNKS[1])
        t.end, t.end_snap = b.capture(), sh.snapshot(b, n)
        t.end_again = b.capture()
        t.end_reversed = b.capture(list(range(n))[::-1])
        t.dicts = [b.q_dict(e) for e in range(n)]
        t.q_dicts = b.q_dicts()
        b.close()
        # the preconditions of every resume check: the capture point lies inside an episode, the second leg ends one,
        # and it changes every env's table
        assert (head(t.mid, "elapsed") > 0).any()
        assert (head(t.end, "ep_t") >= 1).all(), head(t.end, "ep_t")
        for e in range(n):
            assert not qf.same_bits(t.mid_snap[e][0], t.end_snap[e][0]), f"env {e}: the second leg wrote no cell"
        _twins[k] = t
    return _twins[k]


def other_twin(lib, c, key=""):
    """The end snapshot of the batch a restore goes into, left alone: seeds + SHIFT, step(PRE), step(CHUNKS[1])."""
    k = (lib.path, c.name, key, "other")
    if k not in _twins:
        b = begin(make(c, lib, shift=SHIFT), PRE, CHUNKS[1])
        _twins[k] = sh.snapshot(b, b.E)
        b.close()
    return _twins[k]


# ---- 1. resume -----------------------------------------------------------------------------------------------------
def check_resume(lib, c, tmp_path, key=""):
    t = twin(lib, c, key)
    path = tmp_path / "state.npz"
    t.mid.save(path)
    loaded = runtime.BatchState.load(path)
    assert not same_state(loaded, t.mid)
    b = begin(make(c, lib, shift=SHIFT), PRE)   # other seeds, its own rows and random stream
    b.restore(loaded)
    assert b.seeds == t.seeds
    b.curve_begin(1, 4, ring=CHUNKS[1] + 1)   # a curve starts on a restored batch as on any other
    step(b, CHUNKS[1])
    # (an episode is cut after 41 decisions: every env ends one within the 55 of this leg)
    assert (b.curve()["episodes"] == head(t.end, "ep_t")).all() and b.curve()["count"].sum() >= b.E
    assert not mismatches(b, t.end_snap), mismatches(b, t.end_snap)
    assert not same_state(b.capture(), t.end), same_state(b.capture(), t.end)
    b.close()


# ---- 3. the live-row rule ------------------------------------------------------------------------------------------
def blocks(cm):
    """(first row id, rows, cells per row, first cell) of every Q block, in block order."""
    A = cm.arrays
    return [(int(A["row_base"][4 * s + i]), (1 << len(cm.ports[s])) * cm.K * 3, int(A["q_w"][4 * s + i]),
             int(A["q_off"][4 * s + i])) for s in range(cm.S) for i in range(len(cm.ports[s]))]


def live_rows(cm, default_q, q, touched):
    """The rule restated: (row ids, cells as uint64) of one env's dense block and key set."""
    dflt = np.array([default_q], np.float64).view(np.uint64)[0]
    bits = np.unpackbits(touched.view(np.uint8), bitorder="little")[:cm.rows_per_env].astype(bool)
    qb = q.view(np.uint64)
    ids, cells, at = [], [], 0
    for base, n, w, off in blocks(cm):
        assert base == at, "the blocks tile the row ids in block order (else restate the rule for this map)"
        at = base + n
        blk = qb[off: off + n * w].reshape(n, w)
        on = bits[base: base + n] | (blk != dflt).any(axis=1)
        ids.append(base + np.nonzero(on)[0])
        cells.append(blk[on].reshape(-1))
    assert at == cm.rows_per_env
    return np.concatenate(ids).astype(np.uint32), np.concatenate(cells)


def rule_tables(cm):
    """One (name, Q block, key set) per env of the live-row test, default_q = 0.0."""
    Q, tw = cm.q_per_env, (cm.rows_per_env + 31) // 32
    bl = blocks(cm)
    two = next(b for b in bl if b[2] == 2)
    three = next(b for b in bl if b[2] == 3)
    last = max(bl, key=lambda b: b[0])
    out = []

    def env(name, cells=(), bits=()):
        q, t = np.zeros(Q), np.zeros(tw, np.uint32)
        for i, v in cells:
            q[i] = v
        for r in bits:
            t[r >> 5] |= np.uint32(1 << (r & 31))
        out.append((name, q, t))

    def cell_of(b, row, col=0):
        return b[3] + row * b[2] + col

    env("cell without key bit", [(cell_of(bl[3], 5, bl[3][2] - 1), 2.5)])
    env("key bit on a default row", bits=[bl[2][0] + 7])
    env("zeros", [(cell_of(bl[1], 0), -0.0), (cell_of(bl[1], 9), 5e-324), (cell_of(bl[1], 4), 0.0)])
    env("first and last row", [(0, 1.0), (Q - 1, -1.0)], bits=[0, cm.rows_per_env - 1])
    env("2- and 3-column blocks",
        [(cell_of(two, 0, 1), 3.0), (cell_of(two, two[1] - 1, 0), 4.0), (cell_of(three, 0, 2), 5.0),
         (cell_of(three, three[1] - 1, 1), 6.0)])
    env("last key-set word", bits=[last[0] + last[1] - 1, (tw - 1) * 32])
    env("all default")
    out.append(("ties",) + qf.table(cm, "ties", 0.0, 7))
    out.append(("zeros profile",) + qf.table(cm, "zeros", 0.0, 8))
    return out


def check_live_rule(lib, c):
    cm = sh.compiled(c.row)
    hp = dict(sh.HP, default_q=0.0)
    tabs = rule_tables(cm)
    b = make(c, lib, n=len(tabs), hp=hp)
    empty = b.capture()   # a fresh handle, before apply_qinit: nothing is live
    assert int(empty.row_off[-1]) == 0 and int(empty.cell_off[-1]) == 0 and not len(empty.row_ids) and not len(empty.cells)
    b.restore(empty)
    for e, (_, q, t) in enumerate(tabs):
        b.set_q_raw(e, q, t)
    s = b.capture()
    for e, (name, q, t) in enumerate(tabs):
        ids, cells = live_rows(cm, 0.0, q, t)
        kt, ki, kc = section(s, e)
        assert qf.same_bits(kt, t), name
        assert qf.same_bits(ki, ids), (name, ki, ids)
        assert qf.same_bits(kc, cells), name
    names = [n for n, _, _ in tabs]
    assert len(section(s, names.index("all default"))[1]) == 0
    zr = section(s, names.index("zeros"))[1]
    assert len(zr) == 2   # -0.0 and 5e-324 are live, +0.0 under a clear bit is not
    assert len(section(s, names.index("cell without key bit"))[1]) == 1
    assert len(section(s, names.index("key bit on a default row"))[1]) == 1
    f = make(c, lib, n=len(tabs), hp=hp, shift=SHIFT)
    f.restore(s)
    for e, (name, q, t) in enumerate(tabs):
        gq, gt = f.q_raw(e)
        assert qf.same_bits(gq, q) and qf.same_bits(gt, t), name
    assert not same_state(f.capture(), s)
    assert not same_state(b.capture(), s)   # 9. two captures of one handle
    b.close()
    f.close()


# ---- 4. subsets and slots ------------------------------------------------------------------------------------------
SUBSET = ([5, 0, 3], [1, 2, 0])   # envs captured, slots restored into
INTO_RUNNING = ([5, 0], [7, 9])


def check_subset(lib, c, key=""):
    t = twin(lib, c, key)
    a = begin(make(c, lib), CHUNKS[0])
    envs, slots = SUBSET
    part = a.capture(envs)
    two = a.capture(INTO_RUNNING[0])
    a.close()
    for k, e in enumerate(envs):   # a subset's sections are the full capture's
        for x, y in zip(section(part, k), section(t.mid, e)):
            assert qf.same_bits(x, y)
        assert qf.same_bits(part.state[k], t.mid.state[e])
    b = begin(make(c, lib, n=len(envs), shift=SHIFT), PRE)
    b.restore(part, into=slots)
    assert [b.seeds[s] for s in slots] == [t.seeds[e] for e in envs]
    step(b, CHUNKS[1])
    assert not mismatches(b, t.end_snap, slots, envs), mismatches(b, t.end_snap, slots, envs)
    b.close()
    # two records into a batch that is itself in the middle of a run: its other envs go on as in their own twin
    other = other_twin(lib, c, key)
    d = begin(make(c, lib, shift=SHIFT), PRE)
    d.restore(two, into=INTO_RUNNING[1])
    step(d, CHUNKS[1])
    assert not mismatches(d, t.end_snap, INTO_RUNNING[1], INTO_RUNNING[0])
    rest = [e for e in range(d.E) if e not in INTO_RUNNING[1]]
    assert not mismatches(d, other, rest), mismatches(d, other, rest)
    d.close()


def check_long_list(lib, n=300):
    """More listed envs than one block of the env scan holds (256): the 5-switch, 1-train map."""
    row = next(r for r in sh.ROWS if r[:2] == (5, 1))
    cm = sh.compiled(row)
    # (the seeds of tests/_shapes.py's cases, repeated: on this one-train map an episode of another seed may never
    # reach a switch, and a step of so many decisions would then not return)
    seeds = [sh.seeds()[e % sh.E_MAX] for e in range(n)]
    b = runtime.Batch(cm, sh.HP, seeds, lib=lib, ntab=sh.NTAB, max_steps=MAX_STEPS)
    begin(b, 12)
    s = b.capture()
    assert len(s) == n and (np.diff(s.row_off.astype(np.int64)) >= 0).all()
    for e in (0, 1, 255, 256, 257, n - 1):
        ids, cells = live_rows(cm, sh.HP["default_q"], *b.q_raw(e))
        _, ki, kc = section(s, e)
        assert qf.same_bits(ki, ids) and qf.same_bits(kc, cells), e
        one = b.capture([e])
        assert all(qf.same_bits(x, y) for x, y in zip(section(one, 0), section(s, e))), e
        assert qf.same_bits(one.state[0], s.state[e])
    assert len({len(section(s, e)[1]) for e in range(n)}) > 1   # (the envs' tables differ)
    b.close()


# ---- 5. hyperparameter groups --------------------------------------------------------------------------------------
def check_groups(lib, c, key=""):
    assert c.hpg
    t = twin(lib, c, key)
    other = other_twin(lib, c, key)
    a = begin(make(c, lib), CHUNKS[0])
    rec = a.capture([2])   # an env of group 0
    a.close()
    d = begin(make(c, lib, shift=SHIFT), PRE)
    try:
        d.restore(rec, into=[3])   # a slot of group 1
    except ValueError as e:
        assert "slot 3" in str(e)
    else:
        raise AssertionError("a record of group 0 went into a slot of group 1")
    d.restore(rec, into=[4])
    step(d, CHUNKS[1])
    assert not mismatches(d, t.end_snap, [4], [2])
    rest = [e for e in range(d.E) if e != 4]
    assert not mismatches(d, other, rest), mismatches(d, other, rest)
    d.close()


# ---- 6. the slot-epoch wrap across a resume -------------------------------------------------------------------------
# max_steps = 7 cuts every episode after 8 decisions (tests/_limits.py): 2,040 decisions precede reset 256, which clears
# the (switch, train) slots.  The capture is taken 4 decisions before it, in episode 254 (0-based) of every env.
EPOCH_MAX_STEPS = 7
EPOCH_CHUNKS = (2036, 60)


def check_epoch_wrap(lib, c):
    a = begin(make(c, lib, max_steps=EPOCH_MAX_STEPS), EPOCH_CHUNKS[0])
    s = a.capture()
    assert (head(s, "ep_t") == 254).all() and (head(s, "epoch") == 255).all(), (head(s, "ep_t"), head(s, "epoch"))
    step(a, EPOCH_CHUNKS[1])
    end, snap = a.capture(), sh.snapshot(a, a.E)
    assert (head(end, "ep_t") >= 257).all() and (head(end, "epoch") < 10).all()
    a.close()
    b = make(c, lib, max_steps=EPOCH_MAX_STEPS, shift=SHIFT)   # a fresh handle: never begun
    b.restore(s)
    step(b, EPOCH_CHUNKS[1])
    assert not mismatches(b, snap), mismatches(b, snap)
    assert not same_state(b.capture(), end)
    b.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------
def refused(b, state, match, into=None):
    """restore raises SflError naming the reason."""
    try:
        b.restore(state, into=into)
    except _lib.SflError as e:
        assert match in str(e), (match, str(e))
    else:
        raise AssertionError(f"restore was not refused ({match})")


def edited(state, **arrays):
    d = {k: getattr(state, k).copy() for k in ARRAYS}
    d.update(arrays)
    return runtime.BatchState(state.fingerprint, state.layout, **d)


def check_refusals(lib, c, key=""):
    """Every refusal on one target batch, which then steps as its twin does."""
    t = twin(lib, c, key)
    other = other_twin(lib, c, key)
    s = t.mid
    d = begin(make(c, lib, shift=SHIFT), PRE)
    n = d.E
    for hp, why in ((dict(sh.HP, gamma=0.9), "gamma"), (dict(sh.HP, default_q=-4.0), "default_q")):
        x = begin(make(c, lib, hp=hp), 3)
        refused(d, x.capture(), "fingerprint")
        x.close()
    refused(d, s, "listed twice", into=[0] * n)
    refused(d, s, "out of range", into=list(range(1, n + 1)))
    ids = s.row_ids.copy()
    ids[int(s.row_off[2]) - 1] = sh.compiled(c.row).rows_per_env
    refused(d, edited(s, row_ids=ids), "rows_per_env")
    ids = s.row_ids.copy()
    ids[1] = ids[0]
    refused(d, edited(s, row_ids=ids), "strictly ascending")
    short = s.cell_off.copy()
    short[1:] -= np.uint64(1)
    refused(d, edited(s, cell_off=short, cells=s.cells[:-1]), "widths")
    refused(d, edited(s, cells=s.cells[:-1]), "end at")
    down = s.row_off.copy()
    down[1], down[2] = s.row_off[2], s.row_off[1]
    refused(d, edited(s, row_off=down), "decrease")
    try:
        d.restore(s, into=[0])
    except ValueError:
        pass
    else:
        raise AssertionError("one slot for many records")
    step(d, CHUNKS[1])
    assert not mismatches(d, other), mismatches(d, other)
    d.close()


def check_other_map(lib, c, other_cell):
    """A record of another map is refused."""
    a = begin(make(other_cell, lib, n=3), 3)
    s = a.capture()
    a.close()
    d = begin(make(c, lib, n=3), 3)
    refused(d, s, "fingerprint")
    step(d, 5)
    d.close()


def check_modes(lib, c):
    """Evaluation handles, external-action mode and graph-partitioned handles take no part."""
    cm = sh.compiled(c.row)
    a = begin(make(c, lib, n=2), 3)
    s = a.capture()
    ev = runtime.EvalBatch(cm, sh.HP, sh.seeds(2), 1, lib=lib, max_steps=MAX_STEPS)
    d = _lib.StateDesc()
    import ctypes as C
    assert lib.dll.sfl_state_info(ev.h, C.byref(d)) != 0 and "evaluation handle" in lib.dll.sfl_last_error().decode()
    off = np.zeros(3, np.uint64)
    ids = np.arange(2, dtype=np.uint32)
    P = C.POINTER

    def capture_refused(h, match):
        rc = lib.dll.sfl_state_capture(h, 2, ids.ctypes.data_as(P(C.c_uint32)), off.ctypes.data_as(P(C.c_uint64)),
                                       off.ctypes.data_as(P(C.c_uint64)))
        assert rc != 0 and match in lib.dll.sfl_last_error().decode(), lib.dll.sfl_last_error().decode()

    capture_refused(ev.h, "evaluation handle")
    ev.close()
    lib.check(lib.dll.sfl_env_begin(a.h), "sfl_env_begin")
    capture_refused(a.h, "external-action")
    refused(a, s, "external-action")
    a.close()
    p = make(c, lib, n=2)
    owner = np.zeros(cm.S, np.int32)
    lib.check(lib.dll.sfl_part_config(p.h, 0, 1, owner.ctypes.data_as(P(C.c_int32)), 0, 2, 2, 64), "sfl_part_config")
    capture_refused(p.h, "graph-partitioned")
    refused(p, s, "graph-partitioned")
    p.close()
    f = make(c, lib, n=2)
    assert lib.dll.sfl_state_read(f.h, None, None, None, None) != 0
    assert "no pending capture" in lib.dll.sfl_last_error().decode()
    f.close()


# ---- 8. the dict path, 9. determinism --------------------------------------------------------------------------------
def check_dicts(lib, c, key=""):
    t = twin(lib, c, key)
    assert len(t.q_dicts) == t.n
    for e in range(t.n):
        assert list(t.q_dicts[e]) == list(t.dicts[e]), e                     # the same rows in the same order
        assert qf.dict_bits(t.q_dicts[e]) == qf.dict_bits(t.dicts[e]), e


def check_determinism(lib, c, key=""):
    t = twin(lib, c, key)
    assert not same_state(t.end_again, t.end)
    r = t.end_reversed
    for e in range(t.n):
        k = t.n - 1 - e
        assert all(qf.same_bits(x, y) for x, y in zip(section(r, k), section(t.end, e))), e
        assert qf.same_bits(r.state[k], t.end.state[e]) and r.seeds[k] == t.end.seeds[e]


def check_save(lib, c, tmp_path):
    """DistrQLearning.save / q_tables of a multi-env learner: the pickles are byte for byte those of dicts built from
    the dense per-env blocks."""
    import pickle
    envmod = importlib.import_module("network-distributed-q-learning_amd.env")
    dq = importlib.import_module("network-distributed-q-learning_amd.distr_q")
    env = envmod.ASyncSwitchEnv(sh.scenario(c.row), max_steps=MAX_STEPS, n_envs=5)
    model = dq.DistrQLearning(env, seed=300, lib=lib, **sh.HP)
    b = begin(model.batch, CHUNKS[0])

    def dense(envs):
        return [runtime.raw_to_dict(b.cm, sh.HP["default_q"], *b.q_raw(e)) for e in envs]

    for name, envs in (("all.pkl", None), ("some.pkl", [3, 1]), ("one.pkl", [2])):
        model.save(str(tmp_path / name), envs=envs)
        want = dense(range(5) if envs is None else envs)
        want = want[0] if len(want) == 1 else want
        assert (tmp_path / name).read_bytes() == pickle.dumps(want), name
    assert pickle.dumps(model.q_tables()) == pickle.dumps(dense(range(5)))
    b.close()
