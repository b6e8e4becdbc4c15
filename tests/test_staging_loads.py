"""CPU twin of tests/test_staging_loads_gpu.py: the host build alone goes through what each case is for, and
scripts/load_chains.py counts exposed vector-memory round trips as it says it does."""
import importlib.util
import os

import pytest

from tests import _staging as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("c", [c for c in T.CASES if c.G in (16, None)], ids=T.case_id)
def test_no_case_is_vacuous(c):
    T.check_reference(c)


def _load_chains():
    spec = importlib.util.spec_from_file_location("load_chains", os.path.join(ROOT, "scripts", "load_chains.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SERIAL = """\
_Z6k_wavePKvS0_:
\tglobal_load_dwordx2 v[4:5], v[0:1], off
\ts_waitcnt vmcnt(0)
\tv_cmp_gt_f64_e32 vcc, v[4:5], v[2:3]
\tglobal_load_dwordx2 v[6:7], v[0:1], off offset:8
\ts_waitcnt vmcnt(0)
\tv_cmp_gt_f64_e32 vcc, v[6:7], v[2:3]
.Lfunc_end0:
"""
BATCHED = """\
_Z6k_wavePKvS0_:
\tglobal_load_dwordx2 v[4:5], v[0:1], off
\tflat_load_dwordx2 v[6:7], v[0:1]
\ts_waitcnt lgkmcnt(0)
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tv_cmp_gt_f64_e32 vcc, v[4:5], v[2:3]
\ts_waitcnt vmcnt(0)
\tv_cmp_gt_f64_e32 vcc, v[6:7], v[2:3]
\tglobal_store_dwordx2 v[0:1], v[6:7], off
\ts_waitcnt vmcnt(0)
.Lfunc_end0:
_Z9not_oursv:
\tglobal_load_dword v0, v[0:1], off
\ts_waitcnt vmcnt(0)
.Lfunc_end1:
"""


def test_load_chains_counts_a_serial_pair_as_two_and_a_batched_pair_as_one():
    lc = _load_chains()
    serial = lc.chains(SERIAL.splitlines(True))
    assert list(serial) == ["_Z6k_wavePKvS0_"]
    assert lc.summary(serial["_Z6k_wavePKvS0_"]) == {"loop": (2, 2)}
    # one wait for both loads; a wait on lgkmcnt alone, a second wait with no load before it, a store and a kernel
    # that is none of the project's count nothing
    batched = lc.chains(BATCHED.splitlines(True))
    assert list(batched) == ["_Z6k_wavePKvS0_"]
    assert lc.summary(batched["_Z6k_wavePKvS0_"]) == {"loop": (1, 2)}
