"""The sender side of a partitioned round on the MI355X -- the wave kernels' PART staging (k_wave_part, and k_wave2_part
on the 65-train map), k_part_local, k_part_eblk in both directions and k_part_compact with more than one block -- on up
to 8 ranks in one process, against the segment model of tests/_segments.py (A - D), against a twin job on the host
build record for record (E), and against the fused host run (F).

E, lane-per-env body (SFL_KERNEL=scalar: k_part_local, k_part_compact(arrays = 1)): every env's per-round record sets
at the configured capacity equal the host build's byte for byte.

E, wave kernels: the same sets after dropping the MSG_INSERT records on both sides, and without two fields that differ
by design:
  * the group tag in `kind` (length and place): it counts the inserts.  The lane body stages a key-set insert for the
    pending row and one for the current row beside every update (sfl_core.h env_post: q.touch, lines 1194, 1198 and
    1226); the wave kernels let the update record carry the pending row's insert and the owner insert the current row
    when it answers, and stage an insert only for an exploratory decision's row (sfl_wave.h post_part: upd_rec /
    touch_rec, lines 2275-2276 and 2294).
  * the stage number: the lane body counts one stage per arrived train whether or not it has a pending entry
    (sfl_core.h line 1231, ++stage), the wave kernels only the stages that carry records (sfl_wave.h lines 2305 and
    2340).  The owner applies a group's records in stage order, so what is compared is each update's rank among the
    stages of its env's set.
With rows decided in place (local) the wave kernels send other records in other rounds than the host build, which
always sends; E is then not compared (A - D and F are), and the lane body's E still is.

What no test here can pin is the place a record gets on the device: it follows the order of k_part_compact's atomics.
The model checks what must hold under any order."""
import importlib

import pytest

from tests import _segments as sg

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")

# the lane-per-env body on the cases that differ in what k_part_compact(arrays = 1) sees: one rank and two blocks, a
# small k with thousands of deferrals, local rows (which it ignores), episode ends
SCALAR = ("w1-e257", "w2-e64", "w2-e64-local", "w3-e1-episodes")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


def _select(monkeypatch, kernel):
    for k in ("SFL_KERNEL", "SFL_WAVE_G", "SFL_LDS_MAP", "SFL_REQUIRE_WAVE"):
        monkeypatch.delenv(k, raising=False)
    if kernel == "scalar":
        monkeypatch.setenv("SFL_KERNEL", "scalar")


@pytest.mark.parametrize("case", sg.CASES, ids=lambda c: c.name)
def test_wave(lib, monkeypatch, case):
    _select(monkeypatch, "wave")
    got = sg.run_case(case, lib, device="cuda", kernel="wave")
    assert got["variants"] == [sg.variant_of(case)] and got["variants"][0] > 0
    print(case.name, got)


@pytest.mark.parametrize("name", SCALAR)
def test_lane_body(lib, monkeypatch, name):
    _select(monkeypatch, "scalar")
    got = sg.run_case(sg.CASE[name], lib, device="cuda", kernel="scalar")
    assert got["variants"] == [0]
    print(name, got)
