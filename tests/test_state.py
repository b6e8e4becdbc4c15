"""Suspend and resume on the host build (tests/_state.py): a captured batch restored into another batch continues bit
for bit as the run that never stopped; the live-row rule against its numpy restatement; subsets, slots, groups, the
slot-epoch wrap, the refusals, the Q dicts of one capture and DistrQLearning's pickles.  The host build runs the
lane-per-env body only, so every cell here is the `lane` layout class; tests/test_state_gpu.py runs the wave kernels."""
import pytest

from tests import _state as st
from tests import hostsim


@pytest.fixture(scope="module")
def lib():
    return hostsim.lib()


@pytest.mark.parametrize("name", ["krun", "ring", "hpg16"])
def test_resume(lib, tmp_path, name):
    st.check_resume(lib, st.cell(name), tmp_path)


def test_live_row_rule(lib):
    st.check_live_rule(lib, st.cell("g16"))


def test_subsets_and_slots(lib):
    st.check_subset(lib, st.cell("g8"))


def test_env_list_longer_than_a_scan_block(lib):
    st.check_long_list(lib)


def test_groups(lib):
    st.check_groups(lib, st.cell("hpg16"))


def test_epoch_wrap_across_a_resume(lib):
    st.check_epoch_wrap(lib, st.cell("krun"))


def test_refusals(lib):
    st.check_refusals(lib, st.cell("krun"))
    st.check_other_map(lib, st.cell("g16"), st.cell("v7"))
    st.check_modes(lib, st.cell("g16"))


@pytest.mark.parametrize("name", ["krun", "hpg16"])
def test_q_dicts_and_determinism(lib, name):
    st.check_dicts(lib, st.cell(name))
    st.check_determinism(lib, st.cell(name))


def test_save_writes_the_same_pickles(lib, tmp_path):
    st.check_save(lib, st.cell("krun"), tmp_path)
