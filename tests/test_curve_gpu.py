"""Step-mode learning curves on the MI355X (libsfl.so: k_curve_fold behind every step launch): every case of
tests/_curve.py -- each on the kernel family it names, asserted from the handle's counters -- against the same numpy
model of the host build's learn(N) records as tests/test_curve.py, the lifecycle of a curve, and that recording does
not perturb training."""
import importlib

import pytest

from tests import _curve as cv

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


def _select(monkeypatch, case):
    for k in ("SFL_KERNEL", "SFL_WAVE_G", "SFL_LDS_MAP", "SFL_REQUIRE_WAVE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in cv.case_env(case).items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("case", cv.CASES, ids=lambda c: c.name)
def test_case(lib, monkeypatch, case):
    _select(monkeypatch, case)
    cv.run_case(case, lib, check_kernel=True)


@pytest.mark.parametrize("check", cv.LIFECYCLE, ids=lambda f: f.__name__[4:])
def test_lifecycle(lib, monkeypatch, check):
    _select(monkeypatch, cv.LIFE)
    check(lib)


@pytest.mark.parametrize("case", cv.UNCHANGED, ids=lambda c: c.name)
def test_unchanged(lib, monkeypatch, case):
    _select(monkeypatch, case)
    cv.run_unchanged(case, lib)
