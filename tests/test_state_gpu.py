"""Suspend and resume on the MI355X (tests/_state.py): per kernel cell -- the grouped wave kernels at G = 8, 16 (variants
6 and 7), 32, the one-env-per-wavefront kernel with one train slot and with the two-slot ring, the lane-per-env kernel
and the hyperparameter-group kernels -- a batch captured inside an episode, saved, loaded and restored into a batch
that ran on other seeds continues bit for bit as the run that never stopped, and its packed Q rows equal the host
build's.  Then the live-row rule, subsets and slots, groups, the slot-epoch wrap across a resume, the refusals, the Q
dicts of one capture and determinism, on the product library."""
import importlib

import pytest

from tests import _qfuzz as qf
from tests import _state as st
from tests import hostsim

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")
CELL_IDS = [c.name for c in st.CELLS]


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


def _kernel(lib, monkeypatch, c):
    """The cell's kernel settings, and the check that a batch under them runs the kernel the cell names."""
    st.set_env(monkeypatch, c)
    t = st.twin(lib, c)
    assert (t.counters["kernel_variant"], t.counters["group_lanes"]) == qf.EXPECT[c.name] == qf.predict(c), t.counters
    assert t.mid.layout == ("lane" if c.name == "krun" else "wave")
    return t


@pytest.mark.parametrize("name", CELL_IDS)
def test_resume(lib, monkeypatch, tmp_path, name):
    c = st.cell(name)
    _kernel(lib, monkeypatch, c)
    st.check_resume(lib, c, tmp_path)


@pytest.mark.parametrize("name", CELL_IDS)
def test_capture_equals_host_build(lib, monkeypatch, name):
    c = st.cell(name)
    t = _kernel(lib, monkeypatch, c)
    ref = st.twin(hostsim.lib(), c)
    for got, want in ((t.mid, ref.mid), (t.end, ref.end)):
        assert not st.same_state(got, want, st.Q_ARRAYS), st.same_state(got, want, st.Q_ARRAYS)
        assert qf.same_bits(got.seeds, want.seeds) and qf.same_bits(got.sched, want.sched)
        if name == "krun":   # the same layout class: the state records too, and the fingerprint
            assert not st.same_state(got, want), st.same_state(got, want)
    for e in range(t.n):
        assert not qf.same_env_bits(t.end_snap[e], ref.end_snap[e]), e


@pytest.mark.parametrize("name", CELL_IDS)
def test_q_dicts_and_determinism(lib, monkeypatch, name):
    c = st.cell(name)
    _kernel(lib, monkeypatch, c)
    st.check_dicts(lib, c)
    st.check_determinism(lib, c)


def test_live_row_rule(lib, monkeypatch):
    c = st.cell("g16")
    st.set_env(monkeypatch, c)
    st.check_live_rule(lib, c)


def test_subsets_and_slots(lib, monkeypatch):
    c = st.cell("g8")   # 35 envs
    _kernel(lib, monkeypatch, c)
    st.check_subset(lib, c)


def test_env_list_longer_than_a_scan_block(lib, monkeypatch):
    for k in st.KERNEL_ENV:
        monkeypatch.delenv(k, raising=False)
    st.check_long_list(lib)


def test_groups(lib, monkeypatch):
    c = st.cell("hpg16")
    _kernel(lib, monkeypatch, c)
    st.check_groups(lib, c)


@pytest.mark.parametrize("name", ["krun", st.WAVE_CELL])
def test_epoch_wrap_across_a_resume(lib, monkeypatch, name):
    c = st.cell(name)
    st.set_env(monkeypatch, c)
    st.check_epoch_wrap(lib, c)


@pytest.mark.parametrize("name", ["krun", st.WAVE_CELL])
def test_refusals(lib, monkeypatch, name):
    c = st.cell(name)
    _kernel(lib, monkeypatch, c)
    st.check_refusals(lib, c)


def test_refused_maps_and_modes(lib, monkeypatch):
    c = st.cell("g16")
    st.set_env(monkeypatch, c)
    st.check_other_map(lib, c, st.cell("v7"))   # a 16x17 record into a 16x16 handle
    st.check_modes(lib, c)


def test_layout_classes_do_not_mix(lib, monkeypatch):
    """A wave record into an SFL_KERNEL=scalar handle of the same map, and the reverse."""
    c = st.cell("v7")   # the map of the krun cell
    st.set_env(monkeypatch, c)
    w = st.begin(st.make(c, lib, n=3), 5)
    assert w.counters()["kernel_variant"] > 0
    st.set_env(monkeypatch, c, SFL_KERNEL="scalar")
    s = st.begin(st.make(c, lib, n=3), 5)
    assert s.counters()["kernel_variant"] == 0
    ws, ss = w.capture(), s.capture()
    assert (ws.layout, ss.layout) == ("wave", "lane")
    assert not st.same_state(ws, ss, st.Q_ARRAYS)
    st.refused(s, ws, "layout class")
    st.refused(w, ss, "layout class")
    twin = st.begin(st.make(c, lib, n=3), 5, 9)   # (created under SFL_KERNEL=scalar: k_run)
    st.step(s, 9)
    st.step(w, 9)
    ref = st.sh.snapshot(twin, 3)
    assert not st.mismatches(s, ref) and not st.mismatches(w, ref)
    for b in (w, s, twin):
        b.close()
