"""The transition assembler's kernels on the MI355X (k_trans_count / k_trans_write of libsfl.so behind the lane and the
wave env step): after every call the whole ring, total, last_count and dropped bit for bit against a host-build twin
driven by the same actions, which are computed from the twin's outputs.  Batch sizes on both sides of a wavefront and of
one and two 256-env blocks (the cross-block prefix with a last block that is not full), rings of twice the batch and of
five rows (more rows in a call than the ring holds, across block edges), maps with two and four arrived-mask words, the
per-episode clearing, a golden run's update() calls through the GPU library, host and device calls mixed, and the
refused action."""
import importlib

import pytest

from tests import _golden, _transitions as tt, hostsim

pytestmark = pytest.mark.gpu

aec = importlib.import_module("network-distributed-q-learning_amd.aec")
comp = importlib.import_module("network-distributed-q-learning_amd.compiler")
mapgen = importlib.import_module("network-distributed-q-learning_amd.mapgen")
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


def twins(cm, seeds, lib, kernels, **kw):
    """The host-build twin first (its outputs feed the policy), then a GPU batch per kernel."""
    return [aec.AECBatch(cm, seeds, lib=hostsim.lib(), **kw)] + [aec.AECBatch(cm, seeds, lib=lib, kernel=k, **kw) for k in kernels]


def run(bs, cm, calls, N, **kw):
    try:
        rings = tt.drive(bs, cm, calls, N, **kw)
        for b in bs:
            b.sync()
        assert rings[1]["env"].is_cuda and not rings[0]["env"].is_cuda
        return rings
    finally:
        for b in bs:
            b.close()


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("E", [1, 63, 65, 257, 513])
def test_lane_and_wave_equal_the_host_twin(lib, E, small):
    """c2, 150 calls, kernel="lane" and kernel="wave" beside one host twin; N = 2E, or N = 5."""
    cm = comp.compile_scenario(mapgen.make_config("c2"))
    N = 5 if small else 2 * E
    rings = run(twins(cm, [450565 + i for i in range(E)], lib, ("lane", "wave")), cm, 150, N)
    total = int(rings[0]["total"][0])
    assert total > 100 * E  # nearly every call gives every env a row
    if small and E >= 63:
        assert int(rings[0]["last_count"][0]) > N or total > 150 * N


@pytest.mark.parametrize("name", ["grid100x48_s3", "c5_mf"])
def test_more_than_32_trains(lib, name):
    """48 trains (two arrived-mask words) and 128 (four): 9 envs, 80 calls, the wave kernel."""
    cm = comp.compile_scenario(_golden.load(name)["scenario_obj"])
    assert cm.T in (48, 128)
    rings = run(twins(cm, [77 + i for i in range(9)], lib, ("wave",)), cm, 80, 18)
    assert int(rings[0]["total"][0]) > 9 * 40


def test_clearing_33_envs_700_calls(lib):
    """The one-train c1 map at max_steps = 3: every episode is truncated with an entry pending (a 32-bit episode count
    per env clears the table: no narrower counter to wrap)."""
    sc = mapgen.generate(5, 1, 2, seed=mapgen.MAP_SEED, nx_lines=3, ny_lines=3, spacing=6, margin=2, size=18,
                         malfunction=(0.01, 5, 15), name="c1_one_train")
    cm = comp.compile_scenario(sc)
    rings = run(twins(cm, [11 + i for i in range(33)], lib, ("lane",), max_steps=3), cm, 700, 66)
    assert (rings[0]["dropped"] >= 100).all()


def test_golden_replay_c1_through_the_gpu_library(lib):
    g = _golden.load("c1_mf")
    ev = g["learn"]["events"]
    n, rows, _ = tt.replay_golden(g, ev, lib)
    assert n == sum(1 for e in ev if e[0] == "D") and rows == sum(1 for e in ev if e[0] == "U")


def test_host_and_device_calls_mixed(lib):
    """E = 65, 400 calls: step() and step_torch() in blocks of 20, env 1 reset at calls 17 and 40, env 2 without an
    action on every third call; the twin is also checked against the model."""
    cm = comp.compile_scenario(mapgen.make_config("c2"))
    rings = run(twins(cm, [450565 + i for i in range(65)], lib, ("lane", "wave")), cm, 400, 130,
                model=tt.Model(cm, 65, 130), resets={17: 1, 40: 1}, hold=2, mixed=True)
    assert int(rings[0]["dropped"][1]) > 0


def test_refused_action_emits_no_row(lib):
    tt.check_refused_action(lib)
