"""Episodes recorded on the MI355X (runtime.EvalBatch.record / recording / traffic; the rule: include/sfl.h; cases and
the oracle recorder: tests/_record.py): the frame and decision-row stores of every BANK kernel family and of k_run's
bank mode, and the traffic fold of sfl_rec.hip, against the host build on every recorded env and against the Python
oracle on envs 0, 1, 2 and n - 1.  The malfunction counter is compared with both.  No test writes an image."""
import importlib
import subprocess

import numpy as np
import pytest

from tests import _evalbank as eb
from tests import _qfuzz as qf
from tests import _record as rc
from tests import _shapes as sh
from tests import hostsim
from tests.test_eval_diag_gpu import FAMILIES, G32, ROW, SHAPES, Cell, _select

pytestmark = pytest.mark.gpu

runtime = sh.runtime
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")
KRUN = FAMILIES[-1]
BOTH = [G32, KRUN]  # one wave kernel and the lane-per-env body: the two state layout classes


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


@pytest.mark.parametrize("cell", FAMILIES, ids=lambda c: c.name)
def test_oracle_equality(lib, monkeypatch, cell):
    """Case 1 on every kernel family: table (b) at max_steps = 100,000, every env recorded."""
    n = _select(monkeypatch, cell)
    eps = rc.run_device_case(lib, cell.row, n, eb.LONG, "b", expect=cell.expect)
    assert any((ep.state == rc.S_MALF).any() for ep in eps) and all(ep.complete for ep in eps)


@pytest.mark.parametrize("cell", BOTH, ids=lambda c: c.name)
def test_caps(lib, monkeypatch, cell):
    """Case 2: the caps one below, at and one above an env's tick count, one decision and one fewer than all: the kept
    frames and rows (and the traffic fold over them) equal the host build's, which test_record.py holds to the
    uncapped prefix; words past the caps are never written (the neighbouring slot stays intact)."""
    n = _select(monkeypatch, cell)
    full = rc.run_device_case(lib, cell.row, n, eb.LONG, "b", envs=[1, 2], expect=cell.expect)
    Te, De = full[0].ticks, full[0].n_decisions
    for mt, md in ((Te - 1, De), (Te, 1), (Te + 1, De - 1)):
        eps = rc.run_device_case(lib, cell.row, n, eb.LONG, "b", envs=[1, 2], expect=cell.expect, max_ticks=mt, max_decisions=md)
        assert eps[0].complete == (mt >= Te and md >= De) and eps[0].frames == min(mt, Te) and eps[0].rows == min(md, De)
        for k in rc.FRAME_KEYS:
            assert np.array_equal(getattr(eps[1], k), getattr(full[1], k)[:eps[1].frames]), (mt, md, k)


@pytest.mark.parametrize("cell", [FAMILIES[0]] + BOTH, ids=lambda c: c.name)
def test_subset_order_and_unrecorded_twin(lib, monkeypatch, cell):
    """Case 3: [n - 1, 1, 2] recorded -- at G = 16 and G = 32 recorded and unrecorded envs share a wavefront -- and the
    evaluation, the diagnosis and every env's end state equal the twin's, i.e. a run with no recording."""
    n = _select(monkeypatch, cell)
    envs = [n - 1, 1, 2]
    pol = eb.assign(n, "mod")
    t = eb.twin(cell.row, n, pol, qf.MAX_STEPS)
    eps = rc.run_device_case(lib, cell.row, n, qf.MAX_STEPS, "mod", envs=envs, expect=cell.expect)
    assert [ep.env for ep in eps] == envs
    plain = eb.bank(lib, cell.row, n, qf.MAX_STEPS)
    ev, _, out = rc.recorded(lib, cell.row, n, qf.MAX_STEPS, "mod", envs)
    try:
        ref = plain.evaluate(pol)
        assert not eb.mismatches(ev, out, t, pol) and not eb.mismatches(plain, ref, t, pol)
        a, b = ev.diagnose(stall=3), plain.diagnose(stall=3)
        assert all(np.array_equal(a[k], b[k]) for k in ("cls", "blocker", "stalled_for"))
        ev.record([0, n - 1])  # re-arming replaces the recording
        eb.with_pytest_raises(lambda: ev.recording(0), "since the recording was armed")
        out2 = ev.evaluate(pol)
        assert not eb.mismatches(ev, out2, t, pol)
        rc.check_against_oracle(ev, out2, cell.row, pol, qf.MAX_STEPS, [0, n - 1], range(2))
        ev.record(None)
        eb.with_pytest_raises(lambda: ev.recording(0), "no recording armed")
        assert not eb.mismatches(ev, ev.evaluate(pol), t, pol)
    finally:
        ev.close()
        plain.close()


@pytest.mark.parametrize("cell", BOTH, ids=lambda c: c.name)
def test_truncation(lib, monkeypatch, cell):
    """Case 4: table (b) at max_steps = 40: every episode truncated, max_steps + 1 rows."""
    n = _select(monkeypatch, cell)
    eps = rc.run_device_case(lib, cell.row, n, qf.MAX_STEPS, "b", expect=cell.expect)
    assert all(ep.rows == ep.n_decisions == qf.MAX_STEPS + 1 for ep in eps)


@pytest.mark.parametrize("cell", SHAPES, ids=lambda c: c.name)
def test_shapes(lib, monkeypatch, cell):
    """Case 5: table (a) at max_steps = 100,000 on every BANK kernel shape, every env recorded; (16, 17) at G = 16 and
    (64, 65) at G = 64 store a lane's second train slot."""
    n = _select(monkeypatch, cell)
    rc.run_device_case(lib, cell.row, n, eb.LONG, "a", expect=cell.expect)


@pytest.mark.parametrize("cell", BOTH, ids=lambda c: c.name)
def test_traffic(lib, monkeypatch, cell):
    """Case 6: e % 3 with no recorded env on policy 2: the fold equals the host build's and the numpy restatement."""
    n = _select(monkeypatch, cell)
    envs = [e for e in range(n) if e % 3 != 2]
    ev, pol, out = rc.recorded(lib, cell.row, n, eb.LONG, "mod", envs)
    try:
        assert not any(v.any() for v in ev.traffic(2).values()) and ev.traffic(0)["standing"].any()
    finally:
        ev.close()
    rc.run_device_case(lib, cell.row, n, eb.LONG, "mod", envs=envs, expect=cell.expect)


def test_traffic_fold_paths_equal_host(lib, monkeypatch):
    """200 envs on 2 and on 200 policies, every env recorded: many blocks of the fold, and slots alone on their policy;
    the device's traffic equals the host build's for every policy that has a slot."""
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
                ev.record(list(range(n - 1, -1, -1)), max_ticks=60, max_decisions=64)
                ev.evaluate(pol)
                res.append([ev.traffic(p) for p in (range(P) if P == 2 else (0, 1, 77, n - 1))])
            finally:
                ev.close()
        for a, b in zip(*res):
            assert not rc.traffic_mismatches(a, b) and a["occupancy"].any(), P


def test_refusals_and_exports(lib, monkeypatch):
    """Case 10 on the device: the refusals leave the handle usable; both libraries export the entry points."""
    cell = Cell("g8", eb.row(16, 8), 8, expect=(10, 8))
    n = _select(monkeypatch, cell)
    pol = eb.assign(n, "a")
    ev = eb.bank(lib, cell.row, n, eb.LONG)
    try:
        eb.with_pytest_raises(lambda: ev.record([n]), "env")
        eb.with_pytest_raises(lambda: ev.record([1, 1]), "listed twice")
        eb.with_pytest_raises(lambda: ev.record([0], max_ticks=0), "tick_cap")
        eb.with_pytest_raises(lambda: ev.record([0], max_ticks=2**31 - 1, max_decisions=2**31 - 1), "SFL_REC_MAX_BYTES")
        eb.with_pytest_raises(lambda: ev.traffic(0), "no recording armed")
        out = ev.evaluate(pol)
        ev.record([1])
        eb.with_pytest_raises(lambda: ev.recording(0), "sfl_bank_eval")
        again = ev.evaluate(pol)
        assert all(qf.same_bits(out[k], again[k]) for k in eb.OUT_KEYS)
        eb.with_pytest_raises(lambda: ev.recording(1), "slot")
        ms = ev.counters()["last_kernel_ms"]
        ev.traffic(0)
        assert ev.counters()["last_kernel_ms"] == ms and ev.record_ms()[0] > 0.0
    finally:
        ev.close()
    names = ("sfl_bank_record", "sfl_bank_record_info", "sfl_bank_record_counts", "sfl_bank_record_read",
             "sfl_bank_record_traffic", "sfl_bank_record_ms")
    for path in (lib.path, hostsim.lib().path):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
        assert not [x for x in names if x not in exported], path
    assert lib.dll.sfl_abi_version() == 9 == _lib.ABI_VERSION
