"""Step-mode learning curves on the host build (libsfl_hostsim.so: curve_fold_host, the rule as plain loops): every
case of tests/_curve.py against the numpy model of the host build's own learn(N) records, the lifecycle of a curve, and
that recording does not perturb training."""
import pytest

from tests import _curve as cv
from tests import hostsim


@pytest.fixture(scope="module")
def lib():
    return hostsim.lib()


@pytest.mark.parametrize("case", cv.CASES, ids=lambda c: c.name)
def test_case(lib, case):
    cv.run_case(case, lib)


@pytest.mark.parametrize("check", cv.LIFECYCLE, ids=lambda f: f.__name__[4:])
def test_lifecycle(lib, check):
    check(lib)


@pytest.mark.parametrize("case", cv.UNCHANGED, ids=lambda c: c.name)
def test_unchanged(lib, case):
    cv.run_unchanged(case, lib)
