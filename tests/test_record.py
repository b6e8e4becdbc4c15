"""Episodes recorded on the device, on the host build (runtime.EvalBatch.record / recording / traffic, sfl_bank_record*;
the rule: include/sfl.h; cases and the oracle recorder: tests/_record.py): every frame and every decision row against
the Python oracle, the caps, a subset in another order beside an unrecorded handle, truncation, every kernel shape's
map, the traffic fold against its numpy restatement, the AEC path fed with a recorded episode's actions, the renderer,
the refusals and the ABI.

The malfunction counter is compared with the oracle's on every tick: flatland_lite keeps the same counter
(``malfunction_handler.malfunction_down_counter``, decremented at the end of the tick like bits 13-20 of tr_bits)."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _evalbank as eb
from tests import _qfuzz as qf
from tests import _record as rc
from tests import _shapes as sh
from tests import hostsim

runtime = sh.runtime
parity = sh.parity
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
aec = importlib.import_module("network-distributed-q-learning_amd.aec")
render = importlib.import_module("network-distributed-q-learning_amd.render")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4  # seeds 300 to 303
ROW = eb.row(16, 32)


def test_oracle_equality():
    """Case 1: (16, 32, 8), every env on table (b), max_steps = 100,000, all four envs recorded: every frame's cell,
    state, malfunction counter and (on the map) heading, the counts and every decision row equal the oracle's.  On the
    oracle some frame has a train in MALFUNCTION, some train arrives and some train never leaves."""
    os_ = [rc.oracle_episode(ROW, s, 1, eb.LONG) for s in qf.seeds(N)]
    assert any((o.state == rc.S_MALF).any() for o in os_), "precondition (oracle): a train in MALFUNCTION"
    assert any((o.state[-1] == rc.S_DONE).any() for o in os_), "precondition (oracle): a train arrives"
    assert any((o.cell < 0).all(axis=0)[o.state[-1] != rc.S_DONE].any() for o in os_), "precondition (oracle): a train never leaves"
    ev, pol, out = rc.recorded(hostsim.lib(), ROW, N, eb.LONG, "b", list(range(N)))
    try:
        assert ev.record_info() == dict(n=N, tick_cap=sh.scenario(ROW).max_episode_steps, dec_cap=4096, dec_words=10)
        got = rc.check_against_oracle(ev, out, ROW, pol, eb.LONG, list(range(N)), range(N))
        assert [got[k] is os_[k] for k in range(N)] == [True] * N
        for k in range(N):
            ep = ev.recording(k)
            assert ep.complete and ep.frames == ep.ticks and ep.rows == ep.n_decisions
            assert ep.state.dtype == ep.heading.dtype == ep.malfunction.dtype == np.uint8
    finally:
        ev.close()


def test_caps():
    """Case 2: one env with T_e ticks at max_ticks = T_e - 1, T_e, T_e + 1 and max_decisions = 1 and the decision
    count: the kept rows are the uncapped recording's prefix, and `complete` says whether anything was cut."""
    ev, pol, out = rc.recorded(hostsim.lib(), ROW, N, eb.LONG, "b", [1])
    try:
        full = ev.recording(0)
        Te, De = full.ticks, full.n_decisions
        assert full.complete and Te > 2 and De > 1
        for mt, md in ((Te - 1, De), (Te, De), (Te + 1, De), (Te, 1), (Te - 1, 1), (Te + 1, De - 1)):
            ev.record([1], max_ticks=mt, max_decisions=md)
            out2 = ev.evaluate(pol)
            assert all(qf.same_bits(out[k], out2[k]) for k in eb.OUT_KEYS)
            ep = ev.recording(0)
            assert (ep.ticks, ep.n_decisions, ep.tick_cap, ep.dec_cap) == (Te, De, mt, md)
            assert ep.complete == (mt >= Te and md >= De)
            assert ep.frames == min(mt, Te) and ep.rows == min(md, De)
            for k in rc.FRAME_KEYS:
                assert np.array_equal(getattr(ep, k), getattr(full, k)[:ep.frames]), (mt, md, k)
            for k in _lib.REC_DEC_FIELDS:
                assert np.array_equal(ep.decisions[k], full.decisions[k][:ep.rows]), (mt, md, k)
            assert ep.decisions["obs"] == full.decisions["obs"][:ep.rows]
            bad = rc.oracle_mismatches(ev.cm, ep, rc.oracle_episode(ROW, qf.seeds(N)[1], 1, eb.LONG), mt, md)
            assert not bad, (mt, md, bad)
    finally:
        ev.close()


def test_subset_order_and_unrecorded_twin():
    """Case 3: envs [n - 1, 1, 2] of n recorded: the slots map to those envs; evaluate(), diagnose() and every env's end
    state are bit-equal to a handle with no recording; re-arming replaces the recording; disarming makes recording()
    raise."""
    n = 6
    envs = [n - 1, 1, 2]
    pol = eb.assign(n, "mod")
    t = eb.twin(ROW, n, pol, qf.MAX_STEPS)
    plain = eb.bank(hostsim.lib(), ROW, n, qf.MAX_STEPS)
    ev, _, out = rc.recorded(hostsim.lib(), ROW, n, qf.MAX_STEPS, "mod", envs)
    try:
        ref = plain.evaluate(pol)
        assert not eb.mismatches(ev, out, t, pol) and not eb.mismatches(plain, ref, t, pol)
        a, b = ev.diagnose(stall=3), plain.diagnose(stall=3)
        assert all(np.array_equal(a[k], b[k]) for k in ("cls", "blocker", "stalled_for"))
        assert all(np.array_equal(a["table"][k], b["table"][k]) for k in _lib.DIAG_FIELDS)
        rc.check_against_oracle(ev, out, ROW, pol, qf.MAX_STEPS, envs, range(3))
        assert [ev.recording(k).env for k in range(3)] == envs
        ev.record([0, n - 1])  # re-arming replaces the recording
        eb.with_pytest_raises(lambda: ev.recording(0), "since the recording was armed")
        out2 = ev.evaluate(pol)
        assert not eb.mismatches(ev, out2, t, pol)
        rc.check_against_oracle(ev, out2, ROW, pol, qf.MAX_STEPS, [0, n - 1], range(2))
        eb.with_pytest_raises(lambda: ev.recording(2), "slot")
        ev.record(None)
        assert ev.record_info()["n"] == 0
        eb.with_pytest_raises(lambda: ev.recording(0), "no recording armed")
        assert not eb.mismatches(ev, ev.evaluate(pol), t, pol)
    finally:
        ev.close()
        plain.close()


def test_truncation():
    """Case 4: table (b) at max_steps = 40: a truncated episode's rows stop at max_steps + 1 decisions."""
    ev, pol, out = rc.recorded(hostsim.lib(), ROW, N, qf.MAX_STEPS, "b", list(range(N)))
    try:
        assert out["truncated"].all()
        os_ = rc.check_against_oracle(ev, out, ROW, pol, qf.MAX_STEPS, list(range(N)), range(N))
        for k in range(N):
            ep = ev.recording(k)
            assert os_[k].truncated and ep.complete and ep.rows == ep.n_decisions == qf.MAX_STEPS + 1
    finally:
        ev.close()


SHAPES = [(5, 1), (16, 17), (64, 33), (64, 65), (128, 65), pytest.param(257, 64, marks=pytest.mark.slow)]


@pytest.mark.parametrize("S,T", SHAPES)
def test_shapes(S, T):
    """Case 5: table (a) at max_steps = 100,000 on the map of every kernel shape, all envs against the oracle."""
    rw = eb.row(S, T)
    ev, pol, out = rc.recorded(hostsim.lib(), rw, N, eb.LONG, "a", list(range(N)))
    try:
        rc.check_against_oracle(ev, out, rw, pol, eb.LONG, list(range(N)), range(N))
    finally:
        ev.close()


def test_traffic():
    """Case 6: traffic(p) equals the numpy restatement from recording(k) for P = 3 with e % 3; a policy no recorded env
    follows gives zeros; occupancy.sum() is the count of on-map train-frames; `standing` is non-zero."""
    n = 7
    envs = [e for e in range(n) if e % 3 != 2]  # (no recorded env follows policy 2)
    ev, pol, out = rc.recorded(hostsim.lib(), ROW, n, eb.LONG, "mod", envs)
    try:
        eps = [ev.recording(k) for k in range(len(envs))]
        assert [ep.policy for ep in eps] == [e % 3 for e in envs]
        for p in range(3):
            got = ev.traffic(p)
            mine = [ep for ep in eps if ep.policy == p]
            assert not rc.traffic_mismatches(got, rc.restate_traffic(ev.cm, mine)), p
            assert int(got["occupancy"].sum()) == sum(int((ep.cell >= 0).sum()) for ep in mine)
            assert int(got["decisions"].sum()) == sum(ep.rows for ep in mine)
            if p == 2:
                assert not any(v.any() for v in got.values())
            else:
                assert got["standing"].any() and (got["standing"] <= got["occupancy"]).all()
                assert (got["standing_malfunction"] <= got["standing"]).all() and (got["stops"] <= got["decisions"]).all()
        assert ev.traffic(1)["standing_malfunction"].any(), "precondition: a train stands in MALFUNCTION"
        assert ev.record_ms() == (0.0, 0.0)  # (the host build has no device time)
        # capped: only the kept frames and rows count
        ev.record(envs, max_ticks=9, max_decisions=5)
        ev.evaluate(pol)
        eps = [ev.recording(k) for k in range(len(envs))]
        assert all(ep.frames == 9 and ep.rows == 5 for ep in eps)
        for p in range(3):
            assert not rc.traffic_mismatches(ev.traffic(p), rc.restate_traffic(ev.cm, [ep for ep in eps if ep.policy == p])), p
    finally:
        ev.close()


def test_aec_emits_the_recorded_rows():
    """Case 7: a recorded episode's actions fed into aec.AECBatch (same map, seed, max_steps) step by step: every
    (agent, train, state, mask, reward, now) it emits, and every step's (next_switch, step_now), equals the recorded
    row."""
    ev, pol, out = rc.recorded(hostsim.lib(), ROW, N, eb.LONG, "b", [2])
    try:
        ep = ev.recording(0)
    finally:
        ev.close()
    assert ep.complete and ep.rows > 100
    d = ep.decisions
    a = aec.AECBatch(sh.compiled(ROW), [ep.seed], lib=hostsim.lib(), max_steps=eb.LONG)
    try:
        o = a.step(None)
        for i in range(ep.rows):
            got = tuple(int(o[k][0]) for k in ("agent", "train", "slot", "state", "mask", "reward", "now"))
            want = tuple(int(d[k][i]) for k in ("switch", "train", "slot", "state", "mask", "reward", "now"))
            assert got == want, (i, got, want)
            o = a.step([int(d["action"][i])])
            assert (int(o["next_switch"][0]), int(o["step_now"][0])) == (int(d["next_switch"][i]), int(d["step_now"][i])), i
        assert int(o["agent"][0]) == -1  # the episode ended with the last recorded decision
    finally:
        a.close()


def test_episode_save_load(tmp_path):
    ev, pol, out = rc.recorded(hostsim.lib(), ROW, N, eb.LONG, "b", [3], max_ticks=50)
    try:
        ep = ev.recording(0)
    finally:
        ev.close()
    ep.save(tmp_path / "ep.npz")
    assert sorted(os.listdir(tmp_path)) == ["ep.npz"]
    back = runtime.Episode.load(tmp_path / "ep.npz")
    assert not rc.episode_mismatches(back, ep) and back.complete == ep.complete is False


def test_renderer():
    """Case 8: every on-map train's marker centre has its colour and no other train's colour appears in its cell; a
    train off the map paints nothing; frame() is pure; rail_image paints no rail pixel in an empty cell."""
    cm = sh.compiled(ROW)
    ev, pol, out = rc.recorded(hostsim.lib(), ROW, N, eb.LONG, "b", [0])
    try:
        ep = ev.recording(0)
    finally:
        ev.close()
    px = 8
    base = render.rail_image(cm, px)
    assert base.dtype == np.uint8 and base.shape == (cm.H * px, cm.W * px, 3)
    grid = cm.arrays["grid"].reshape(cm.H, cm.W)
    cells = base.reshape(cm.H, px, cm.W, px, 3).transpose(0, 2, 1, 3, 4)
    assert (cells[grid == 0] == np.array(render.BACKGROUND, np.uint8)).all()
    assert all((cells[r, c] == np.array(render.RAIL, np.uint8)).all(axis=-1).any() for r, c in zip(*np.nonzero(grid)))
    t = int(np.argmax((ep.cell >= 0).sum(axis=1)))  # the frame with the most trains on the map
    on = np.nonzero(ep.cell[t] >= 0)[0]
    assert len(on) >= 2 and (ep.cell[t] < 0).any()
    img = render.frame(cm, ep, t, cell_px=px)
    assert img.dtype == np.uint8 and img.shape == base.shape and np.array_equal(img, render.frame(cm, ep, t, cell_px=px))
    colours = {h: np.array(render.train_colour(h), np.uint8) for h in range(cm.T)}
    fc = img.reshape(cm.H, px, cm.W, px, 3).transpose(0, 2, 1, 3, 4)
    for h in on:
        r, c = divmod(int(ep.cell[t, h]), cm.W)
        assert (img[r * px + px // 2, c * px + px // 2] == colours[h]).all(), h
        for g in range(cm.T):
            if g != h:
                assert not (fc[r, c] == colours[g]).all(axis=-1).any(), (h, g)
    # a train off the map paints nothing: the cells without a train are the rail image's
    held = np.zeros((cm.H, cm.W), bool)
    held[np.divmod(ep.cell[t, on], cm.W)] = True
    assert np.array_equal(fc[~held], cells[~held])
    off = runtime.Episode(0, 0, 0, 1, 0, 1, 1, -np.ones((1, cm.T), np.int32), np.zeros((1, cm.T), np.uint8),
                          np.zeros((1, cm.T), np.uint8), np.zeros((1, cm.T), np.uint8), ep.decisions)
    assert np.array_equal(render.frame(cm, off, 0, cell_px=px), base)
    # a malfunctioning train is outlined, the deciding switch of a decision is highlighted
    tm, hm = [int(x[0]) for x in np.nonzero(ep.state == rc.S_MALF)]
    r, c = divmod(int(ep.cell[tm, hm]), cm.W)
    assert (render.frame(cm, ep, tm, cell_px=px)[r * px, c * px] == np.array(render.MALFUNCTION, np.uint8)).all()
    sr, sc = cm.switch_ids[int(ep.decisions["switch"][0])]
    with_d = render.frame(cm, ep, 0, decision=0, cell_px=px)
    assert (with_d[sr * px, sc * px] == np.array(render.DECIDING, np.uint8)).all()
    frames = list(render.frames_at_decisions(cm, ep, cell_px=px))
    assert len(frames) == ep.rows and all(f.shape == base.shape for f in frames[:3])


def test_save_png(tmp_path):
    rgb = render.rail_image(sh.compiled(eb.row(5, 1)), 4)
    render.save_png(tmp_path / "a.png", rgb)
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(tmp_path / "a.png").convert("RGB")), rgb)


def test_refusals_and_abi():
    """Case 10: each refusal leaves the handle usable; version 9; the new names in the header, _lib.EXPORTS and both
    libraries' dynamic symbols; the struct sizes."""
    import ctypes as C
    lib = hostsim.lib()
    pol = eb.assign(N, "a")
    ev = eb.bank(lib, ROW, N, qf.MAX_STEPS)
    b = runtime.Batch(sh.compiled(ROW), sh.HP, [1], lib=lib, ntab=sh.NTAB)
    try:
        one = np.array([0], np.uint32)
        assert lib.dll.sfl_bank_record(b.h, 1, one.ctypes.data_as(C.POINTER(C.c_uint32)), 5, 5) == -1
        assert "not an evaluation handle" in lib.dll.sfl_last_error().decode()
        assert lib.dll.sfl_bank_record_ms(b.h, None, None) == -1 and lib.dll.sfl_bank_record_info(b.h, C.byref(_lib.RecordInfo())) == -1
        eb.with_pytest_raises(lambda: ev.record([N]), f"env {N} of {N}")
        eb.with_pytest_raises(lambda: ev.record([1, 2, 1]), "listed twice")
        eb.with_pytest_raises(lambda: ev.record([0], max_ticks=0), "tick_cap")
        eb.with_pytest_raises(lambda: ev.record([0], max_decisions=0), "dec_cap")
        T = ev.cm.T
        ok_ticks = (_lib.REC_MAX_BYTES - 40) // (T * 8)
        eb.with_pytest_raises(lambda: ev.record([0], max_ticks=ok_ticks + 1, max_decisions=1), "SFL_REC_MAX_BYTES")
        eb.with_pytest_raises(lambda: ev.record([0, 1], max_ticks=2**31 - 1, max_decisions=2**31 - 1), "SFL_REC_MAX_BYTES")
        assert ev.record_info()["n"] == 0
        eb.with_pytest_raises(lambda: ev.traffic(0), "no recording armed")
        ev.record([2, 0])
        eb.with_pytest_raises(lambda: ev.recording(0), "sfl_bank_eval")
        eb.with_pytest_raises(lambda: ev.traffic(0), "sfl_bank_eval")
        out = ev.evaluate(pol)
        eb.with_pytest_raises(lambda: ev.recording(2), "slot 2 of 2")
        eb.with_pytest_raises(lambda: ev.traffic(eb.P), "policy")
        eb.with_pytest_raises(lambda: ev.record([0, 0]), "listed twice")  # (a refused arming leaves the armed one)
        assert ev.record_info()["n"] == 2 and ev.recording(0).env == 2
        assert not eb.mismatches(ev, out, eb.twin(ROW, N, pol, qf.MAX_STEPS), pol)
    finally:
        ev.close()
        b.close()
    names = ("sfl_bank_record", "sfl_bank_record_info", "sfl_bank_record_counts", "sfl_bank_record_read",
             "sfl_bank_record_traffic", "sfl_bank_record_ms")
    hdr = open(os.path.join(REPO, "include", "sfl.h")).read()
    assert int(re.search(r"#define\s+SFL_ABI_VERSION\s+(\d+)", hdr).group(1)) == 9 == _lib.ABI_VERSION == lib.dll.sfl_abi_version()
    assert int(re.search(r"#define\s+SFL_REC_DEC_WORDS\s+(\d+)", hdr).group(1)) == len(_lib.REC_DEC_FIELDS) == 10
    assert re.search(r"#define\s+SFL_REC_MAX_BYTES\s+\(1ull << 30\)", hdr) and _lib.REC_MAX_BYTES == 1 << 30
    for x in names:
        assert re.search(r"^int\s+" + x + r"\s*\(", hdr, flags=re.M) and x in _lib.EXPORTS, x
    syms = subprocess.run(["nm", "-D", "--defined-only", lib.path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    assert not [x for x in names if x not in exported]
    assert C.sizeof(_lib.RecordInfo) == 16 and C.sizeof(_lib.RecordTraffic) == 5 * C.sizeof(C.c_void_p)
