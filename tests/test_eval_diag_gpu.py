"""The non-arrival diagnosis of policy-bank evaluation on the MI355X (runtime.EvalBatch.diagnose / hotspots; the rule:
include/sfl.h; cases and the oracle restatement: tests/_diag.py): the last-move record of every BANK kernel family and
of k_run's bank mode, and the kernels of sfl_diag.hip in both state layout classes, against the host build on every env
and against the Python oracle on the first three and the last env."""
import importlib
import subprocess
from collections import namedtuple

import numpy as np
import pytest

from tests import _diag as dg
from tests import _evalbank as eb
from tests import _qfuzz as qf
from tests import _shapes as sh
from tests import hostsim

pytestmark = pytest.mark.gpu

runtime = sh.runtime
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")

# expect: (kernel_variant, group_lanes)
Cell = namedtuple("Cell", "name row G env expect", defaults=((), None))
ROW = eb.row(16, 32)
# case 1's map on every kernel family that holds it
FAMILIES = (
    Cell("g16", ROW, 16, expect=(7, 16)),      # two train slots per lane in a group of 16
    Cell("g32", ROW, 32, expect=(8, 32)),
    Cell("g64", ROW, 64, expect=(1, 64)),
    Cell("lm", eb.row(16, 32, 3), 32, expect=(11, 32)),   # the map tables in LDS: a BANK kernel of its own
    Cell("krun", ROW, None, (("SFL_KERNEL", "scalar"),), (0, 1)),   # the lane-per-env body: the [T][E] state layout
)
# case 7
SHAPES = (
    Cell("5x1", eb.row(5, 1), 8, expect=(10, 8)),          # T = 1: no blocker possible
    Cell("16x17", eb.row(16, 17), 16, expect=(7, 16)),     # first train in the second slot at G = 16
    Cell("64x33", eb.row(64, 33), 64, expect=(3, 64)),
    Cell("64x65", eb.row(64, 65), 64, expect=(5, 64)),     # second slot at one env per wavefront
    Cell("128x65", eb.row(128, 65), 64, expect=(5, 64)),
)
G32 = FAMILIES[1]


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


def _select(monkeypatch, cell):
    for k in ("SFL_KERNEL", "SFL_WAVE_G", "SFL_LDS_MAP", "SFL_REQUIRE_WAVE"):
        monkeypatch.delenv(k, raising=False)
    env = dict(cell.env)
    if cell.G is not None:
        env["SFL_WAVE_G"] = str(cell.G)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cm = sh.compiled(cell.row)
    n = sh.n_envs(cell.G)
    v = sh.choose_variant(cm.S, cm.T, n, sh.lm_bytes(cm.H, cm.W, cm.K), env)
    assert (v, sh.group_lanes(v)) == cell.expect, (cell.name, v)
    return n


@pytest.mark.parametrize("cell", FAMILIES, ids=lambda c: c.name)
def test_oracle_equality_all_classes(lib, monkeypatch, cell):
    """Case 1 on every kernel family: table (b) at max_steps = 100,000, stall 3 and 10; classes 2 to 6 all occur on the
    oracle's four envs of the (16, 32, 8) map."""
    n = _select(monkeypatch, cell)
    if cell.row == ROW:
        ds = [dg.oracle_diag(ROW, s, 1, eb.LONG, 3) for s in qf.seeds(4)]
        assert all(dg.oracle_counts(ds)[c] > 0 for c in range(2, 7))
    dg.run_device_case(lib, cell.row, n, eb.LONG, "b", (3, 10), cell.expect)


def test_truncation(lib, monkeypatch):
    """Case 2: every episode truncated, and truncated beside untruncated episodes in one batch."""
    n = _select(monkeypatch, G32)
    dg.run_device_case(lib, ROW, n, qf.MAX_STEPS, "b", (3,), G32.expect)
    cell = Cell("g8", eb.row(16, 8), 8, expect=(10, 8))
    _select(monkeypatch, cell)
    t40 = eb.twin(cell.row, 35, eb.assign(35, "ab"), qf.MAX_STEPS)
    assert t40.truncated.any() and not t40.truncated.all(), "precondition (twin): truncated and untruncated episodes"
    dg.run_device_case(lib, cell.row, 35, qf.MAX_STEPS, "ab", (3,), cell.expect)


def test_mostly_arriving(lib, monkeypatch):
    """Case 3: (16, 8, 8) on table (a)."""
    cell = Cell("g8", eb.row(16, 8), 8, expect=(10, 8))
    n = _select(monkeypatch, cell)
    c = dg.oracle_counts([dg.oracle_diag(cell.row, s, 0, eb.LONG, 30) for s in qf.seeds(4)])
    assert c[dg.ARRIVED] > 0 and c[1:].sum() > 0
    dg.run_device_case(lib, cell.row, n, eb.LONG, "a", (30,), cell.expect)


@pytest.mark.parametrize("cell", [G32, FAMILIES[-1]], ids=lambda c: c.name)
def test_every_window_edge(lib, monkeypatch, cell):
    """Case 4, in both state layout classes: stall 1 to 12 and a window longer than every episode on one evaluation;
    afterwards the evaluation's outputs and every env's state are what they were."""
    n = _select(monkeypatch, cell)
    pol = tuple(1 for _ in range(n))
    t = eb.twin(ROW, n, pol, eb.LONG)
    host_ev, _, _ = dg.evaluated(hostsim.lib(), ROW, n, eb.LONG, "b")
    ev = None
    try:
        ev, pol, out = dg.evaluated(lib, ROW, n, eb.LONG, "b")
        assert not eb.mismatches(ev, out, t, pol)
        for s in list(range(1, 13)) + [int(out["ticks"].max()) + 5]:
            got = ev.diagnose(stall=s)
            dg.check_against_host(ev, got, host_ev, host_ev.diagnose(stall=s))
            dg.check_against_oracle(ev, got, out, ROW, pol, eb.LONG, s, envs=(0, 1, 2, n - 1))
        bad = eb.mismatches(ev, out, t, pol)
        assert not bad, bad[:8]
    finally:
        host_ev.close()
        if ev is not None:
            ev.close()


@pytest.mark.parametrize("kind", ["mod", "a"])
def test_per_policy_fold(lib, monkeypatch, kind):
    """Case 5: the device's cells equal the host build's and the numpy restatement from the device's per-train arrays;
    policies without episodes have NaN means; hotspots(p).sum() is p's stalled trains."""
    cell = SHAPES[1]
    n = _select(monkeypatch, cell)
    dg.run_device_case(lib, cell.row, n, eb.LONG, kind, (5,), cell.expect)
    ev, pol, out = dg.evaluated(lib, cell.row, n, eb.LONG, kind)
    try:
        got = ev.diagnose(stall=5)
        t = got["table"]
        assert not dg.table_mismatches(t, dg.restate_cells(got, out["ticks"], 5, pol, ev.P), ev.cm.T)
        arrived = np.array([(got["cls"][:, np.asarray(pol) == p] == dg.ARRIVED).sum() for p in range(ev.P)])
        assert np.array_equal(sum(t[k] for k in _lib.DIAG_CLASSES[1:]) + arrived, t["episodes"] * ev.cm.T)
        assert np.isnan(t["jammed_frac"][t["episodes"] == 0]).all() and (kind != "a" or t["episodes"].tolist() == [n, 0, 0])
        for p in range(ev.P):
            assert int(ev.hotspots(p).sum()) == int(t["stop_loop"][p] + t["deadlock_queue"][p] + t["deadlock_cycle"][p])
    finally:
        ev.close()


def test_fold_paths_equal_host(lib, monkeypatch):
    """The fold's two paths (the wave reduction; lanes alone on their policy) and many blocks of the classify pass: 200
    envs on 2 and on 200 policies, the device's cells and hotspots equal the host build's."""
    cell = Cell("g8", eb.row(16, 8), 8, expect=(10, 8))
    _select(monkeypatch, cell)
    n = 200
    tabs = eb.tables(cell.row)
    for P, pol in ((2, [0 if e % 5 else 1 for e in range(n)]), (n, list(range(n)))):
        res = []
        for L in (lib, hostsim.lib()):
            ev = runtime.EvalBatch(sh.compiled(cell.row), sh.HP, qf.seeds(n), P, lib=L, max_steps=eb.LONG)
            try:
                for p in range(P):
                    ev.set_policy_raw(p, *tabs[p % 2])
                ev.evaluate(pol)
                got = ev.diagnose(stall=4)
                res.append((got, np.stack([ev.hotspots(p) for p in range(P)])))
            finally:
                ev.close()
        assert all(np.array_equal(res[0][0][k], res[1][0][k]) for k in ("cls", "blocker", "stalled_for"))
        assert all(np.array_equal(res[0][0]["table"][k], res[1][0]["table"][k]) for k in _lib.DIAG_FIELDS), P
        assert np.array_equal(res[0][1], res[1][1]) and res[0][0]["table"]["episodes"].sum() == n


def test_second_evaluation(lib, monkeypatch):
    """Case 6: nothing of the first evaluation's diagnosis is left in the second's."""
    cell = SHAPES[1]
    n = _select(monkeypatch, cell)
    ev = eb.bank(lib, cell.row, n, eb.LONG)
    try:
        for kind in ("mod", "perm"):
            pol = eb.assign(n, kind)
            out = ev.evaluate(pol)
            dg.check_against_oracle(ev, ev.diagnose(stall=4), out, cell.row, pol, eb.LONG, 4, envs=(0, 1, 2, n - 1))
    finally:
        ev.close()


@pytest.mark.parametrize("cell", SHAPES, ids=lambda c: c.name)
def test_shapes(lib, monkeypatch, cell):
    """Case 7: table (a) at max_steps = 100,000 and table (b) at 40 on every BANK kernel shape."""
    n = _select(monkeypatch, cell)
    dg.run_device_case(lib, cell.row, n, eb.LONG, "a", (3, 30), cell.expect)
    dg.run_device_case(lib, cell.row, n, qf.MAX_STEPS, "b", (3,), cell.expect)


def test_refusals_and_exports(lib, monkeypatch):
    """Case 8 on the device: the refusals leave the handle usable; both libraries export the entry points."""
    cell = Cell("g8", eb.row(16, 8), 8, expect=(10, 8))
    n = _select(monkeypatch, cell)
    ev = eb.bank(lib, cell.row, n, eb.LONG)
    try:
        eb.with_pytest_raises(lambda: ev.diagnose(), "no successful sfl_bank_eval")
        out = ev.evaluate(eb.assign(n, "a"))
        eb.with_pytest_raises(lambda: ev.hotspots(0), "sfl_bank_diag")
        eb.with_pytest_raises(lambda: ev.diagnose(stall=0), "stall")
        first = ev.diagnose(stall=3)
        eb.with_pytest_raises(lambda: ev.hotspots(eb.P), "policy")
        again = ev.evaluate(eb.assign(n, "a"))
        assert all(qf.same_bits(out[k], again[k]) for k in eb.OUT_KEYS)
        assert np.array_equal(ev.diagnose(stall=3)["cls"], first["cls"])
        ms = ev.counters()["last_kernel_ms"]
        ev.diagnose(stall=9)
        assert ev.counters()["last_kernel_ms"] == ms  # (never part of last_kernel_ms)
    finally:
        ev.close()
    names = ("sfl_bank_diag", "sfl_bank_diag_read", "sfl_bank_diag_hot", "sfl_bank_diag_ms")
    for path in (lib.path, hostsim.lib().path):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
        assert not [x for x in names if x not in exported], path
    assert lib.dll.sfl_abi_version() == 9 == _lib.ABI_VERSION
