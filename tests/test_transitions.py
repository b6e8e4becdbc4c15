"""External-action mode's transition assembler (AECBatch.transitions_begin; include/sfl.h sfl_env_trans_*; DESIGN.md
§24) on the host build: pinned to the reference's recorded update() calls, a batch against the plain-Python model of
tests/_transitions.py with rings larger and smaller than a call's output, the per-episode clearing across many resets,
and the guards of the C ABI."""
import ctypes as C
import importlib

import pytest
import torch

from tests import _golden, _transitions as tt, hostsim

aec = importlib.import_module("network-distributed-q-learning_amd.aec")
comp = importlib.import_module("network-distributed-q-learning_amd.compiler")
mapgen = importlib.import_module("network-distributed-q-learning_amd.mapgen")
runtime = importlib.import_module("network-distributed-q-learning_amd.runtime")
part = importlib.import_module("network-distributed-q-learning_amd.partition")
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")

HP = dict(gamma=1.0, epsilon=0.0, epsilon_decay_rate=1.0, lr=0.0, lr_decay_rate=1.0, default_q=0.0)

# (terminal rows, rows with agent == next_agent, most terminal rows behind one decision) of the recorded runs
GOLDEN_STATS = {"c1_mf": (75, 95, 2), "c1_trunc": (13, 15, 2), "c3_mf": (13, 2088, 2), "c2_mf": (99, 523, 1)}


# ---- 1. pinned to the reference --------------------------------------------------------------------------------
def _pinned(name, max_decisions=None):
    g = _golden.load(name)
    assert g["exploit_freq"] is None
    ev = g["learn"]["events"]
    term, same, most = tt.golden_stats(ev)
    assert term > 0 and same > 0, (name, term, same)  # the data itself has terminal rows and STOP rows
    if name in GOLDEN_STATS:
        assert (term, same, most) == GOLDEN_STATS[name], (name, term, same, most)
    if name in ("c1_mf", "c1_trunc", "c3_mf"):
        assert most >= 2  # a decision with two or more bonus rows
    n, rows, dropped = tt.replay_golden(g, ev, hostsim.lib(), max_decisions=max_decisions)
    if max_decisions is None:
        assert n == sum(1 for e in ev if e[0] == "D")
        assert rows == sum(1 for e in ev if e[0] == "U")  # every update() call of the run, and nothing else
    else:
        assert n == max_decisions
    return dropped


@pytest.mark.parametrize("name", ["c1_mf", "c1_nomf", "c1_trunc", "c2_mf", "c3_mf", "city4_mf"])
def test_rows_equal_the_references_update_calls(name):
    """(The two largest replays, c2_mf and c3_mf, take under a second each: no slow mark.)"""
    dropped = _pinned(name)
    if name == "c1_trunc":
        assert dropped > 0  # truncated episodes end with entries pending: dropped and counted


def test_rows_equal_the_references_update_calls_128_trains():
    """c5: 128 trains, four arrived-mask words; the first 300 decisions.  The whole run has up to 4 bonus rows behind
    one decision."""
    g = _golden.load("c5_mf")
    assert comp.compile_scenario(g["scenario_obj"]).T == 128
    assert tt.golden_stats(g["learn"]["events"])[2] <= 4
    _pinned("c5_mf", max_decisions=300)


# ---- 2. a batch against the model ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4096, 64, 7])
def test_batch_against_the_model(N):
    """64 c2 envs, 400 calls: env 1 reset at calls 17 and 40, env 2 without an action on every third call, host and
    device calls alternating in blocks of 20.  N = 7 is smaller than one call's output: only the last 7 rows of a call
    are written.  Every slot of the ring after every call; slots never written keep the test's fill."""
    cm = comp.compile_scenario(mapgen.make_config("c2"))
    E = 64
    b = aec.AECBatch(cm, [450565 + i for i in range(E)], lib=hostsim.lib())
    model = tt.Model(cm, E, N)
    most = 0
    try:
        orig = model.call

        def call(actions, out):
            nonlocal most
            rows = orig(actions, out)
            most = max(most, len(rows))
            return rows

        model.call = call
        tt.drive([b], cm, 400, N, model=model, resets={17: 1, 40: 1}, hold=2, mixed=True)
        b.sync()
    finally:
        b.close()
    assert model.total > 4096 and most > 7 and model.dropped.sum() > 0 and model.dropped[1] > 0
    if N == 4096:
        assert (model.ring["terminal"] == 1).any() and (model.ring["agent"] == model.ring["next_agent"]).any()


# ---- 3. clearing ---------------------------------------------------------------------------------------------
def test_clearing_across_600_resets():
    """One train, max_steps = 3: every episode is truncated with an entry pending.  The table is cleared by an episode
    count of 32 bits per env (no narrower counter to wrap); 600 episode ends, checked against the model on every call."""
    sc = mapgen.generate(5, 1, 2, seed=mapgen.MAP_SEED, nx_lines=3, ny_lines=3, spacing=6, margin=2, size=18,
                         malfunction=(0.01, 5, 15), name="c1_one_train")
    cm = comp.compile_scenario(sc)
    assert cm.T == 1
    b = aec.AECBatch(cm, [11], lib=hostsim.lib(), max_steps=3)
    model = tt.Model(cm, 1, 16)
    try:
        ring = b.transitions_begin(capacity=16)
        tt.fill_ring(ring)
        o = tt.np_out(b.step_torch(None))
        model.call(None, o)
        ends = k = 0
        while ends < 600:
            acts = tt.fixed_policy(cm, o["agent"], o["mask"], k)
            o = tt.np_out(b.step_torch(torch.tensor(acts, dtype=torch.int32)))
            model.call(acts, o)
            model.check(ring, k)
            ends += int(o["agent"][0] < 0)
            k += 1
        assert k < 6000
    finally:
        b.close()
    assert model.dropped[0] >= 300 and model.total > 600


# ---- 4. guards and ABI -----------------------------------------------------------------------------------------
def _io(E, N=8):
    ring = {k: torch.zeros(N, dtype=torch.int32) for k in aec.AECBatch.TRANS_FIELDS}
    ring["terminal"] = torch.zeros(N, dtype=torch.uint8)
    ring["obs"] = torch.zeros((N, tt.W), dtype=torch.int32)
    ring["next_obs"] = torch.zeros((N, tt.W), dtype=torch.int32)
    ring["next_action_mask"] = torch.zeros((N + 1, tt.A), dtype=torch.uint8)
    ring["total"] = torch.zeros(1, dtype=torch.int64)
    ring["last_count"] = torch.zeros(1, dtype=torch.int32)
    ring["dropped"] = torch.zeros(E, dtype=torch.int64)
    io = _lib.EnvTransIO()
    io.capacity = N
    for k, ct in _lib.EnvTransIO._fields_[2:]:
        setattr(io, k, C.cast(ring[k].data_ptr(), ct))
    return ring, io


def test_guards():
    lib = hostsim.lib()
    d = lib.dll
    cm = comp.compile_scenario(mapgen.make_config("c1"))
    ring, io = _io(2)
    plain = runtime.Batch(cm, HP, [1, 2], lib=lib)
    with pytest.raises(_lib.SflError, match="not in external-action mode"):
        lib.check(d.sfl_env_trans_begin(plain.h, C.byref(io)), "sfl_env_trans_begin")
    plain.close()
    ev = runtime.EvalBatch(cm, HP, [1, 2], 1, lib=lib)
    with pytest.raises(_lib.SflError, match="evaluation handle"):
        lib.check(d.sfl_env_trans_begin(ev.h, C.byref(io)), "sfl_env_trans_begin")
    ev.close()
    pb = part.PartitionedBatch(cm, dict(HP, epsilon=0.5, lr=0.1), [1, 2], 0, 2, lib=lib, ntab=4096, buffer_device="cpu")
    with pytest.raises(_lib.SflError, match="graph-partitioned"):
        lib.check(d.sfl_env_trans_begin(pb.batch.h, C.byref(io)), "sfl_env_trans_begin")
    pb.close()
    assert d.sfl_env_trans_begin(None, C.byref(io)) != 0 and "null" in d.sfl_last_error().decode()
    b = aec.AECBatch(cm, [1, 2], lib=lib)
    try:
        for bad in (0, -1, 1 << 31, 2.0, True):
            with pytest.raises(ValueError, match="capacity"):
                b.transitions_begin(capacity=bad)
        io.capacity = 0
        assert d.sfl_env_trans_begin(b.batch.h, C.byref(io)) != 0 and "capacity" in d.sfl_last_error().decode()
        io.capacity = 8
        assert d.sfl_env_trans_begin(b.batch.h, None) != 0 and "null" in d.sfl_last_error().decode()
        assert d.sfl_env_trans_end(b.batch.h) != 0 and "no transition assembler" in d.sfl_last_error().decode()
        # a misaligned mask column is refused before anything runs
        io.next_action_mask = C.cast(ring["next_action_mask"].data_ptr() + 8, _lib.P(C.c_uint8))
        assert d.sfl_env_trans_begin(b.batch.h, C.byref(io)) != 0 and "aligned" in d.sfl_last_error().decode()
        o = b.step_torch(None)
        b.step_torch(torch.tensor(tt.fixed_policy(cm, o["agent"].numpy(), o["mask"].numpy(), 0), dtype=torch.int32))
        assert b.transitions() is None and all(not t.any() for t in ring.values())
        assert b.transitions_begin().keys() == b.transitions().keys() and b.transitions()["env"].numel() == 2 * b.E
    finally:
        b.close()


def test_refused_action_emits_no_row():
    tt.check_refused_action(hostsim.lib())


def test_end_leaves_the_ring_untouched():
    cm = comp.compile_scenario(mapgen.make_config("c2"))
    b = aec.AECBatch(cm, [5, 6, 7], lib=hostsim.lib())
    try:
        ring = b.transitions_begin(capacity=32)
        o = tt.np_out(b.step_torch(None))
        for k in range(40):
            o = tt.np_out(b.step_torch(torch.tensor(tt.fixed_policy(cm, o["agent"], o["mask"], k), dtype=torch.int32)))
        assert int(ring["total"][0]) > 32
        b.transitions_end()
        keep = {k: v.clone() for k, v in ring.items()}
        for k in range(40, 80):
            o = tt.np_out(b.step_torch(torch.tensor(tt.fixed_policy(cm, o["agent"], o["mask"], k), dtype=torch.int32)))
        assert all(torch.equal(ring[k], keep[k]) for k in ring)
        # a new begin starts from an empty table: the first call emits nothing, whatever was pending before
        ring2 = b.transitions_begin(capacity=32)
        o = tt.np_out(b.step_torch(torch.tensor(tt.fixed_policy(cm, o["agent"], o["mask"], 80), dtype=torch.int32)))
        assert int(ring2["total"][0]) == 0 and int(ring2["last_count"][0]) == 0
        assert all(torch.equal(ring[k], keep[k]) for k in ring)
        b.sync()
    finally:
        b.close()


def test_exports_and_abi_version():
    assert {"sfl_env_trans_begin", "sfl_env_trans_end"} <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 9 and hostsim.lib().dll.sfl_abi_version() == 9
    assert aec.DEST_BONUS == _lib.DEST_BONUS == 1000
