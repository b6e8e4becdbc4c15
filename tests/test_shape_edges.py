"""The shape-edge sweep without a GPU: tests/_shapes.py's restatement of csrc/sfl_engine.h's kVariants and
choose_variant against the header itself, the coverage of the (variant x instantiation) matrix by the cases
tests/test_shape_edges_gpu.py runs, and the reference side of every comparison those cases make -- the host build
of the lane body against the oracle on every edge row."""
import importlib
import os
import re

import numpy as np
import pytest

from tests import _shapes as sh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "network-distributed-q-learning_amd", "csrc")
mapgen = importlib.import_module("network-distributed-q-learning_amd.mapgen")
comp = importlib.import_module("network-distributed-q-learning_amd.compiler")

WAVE = range(1, sh.NUM_VARIANTS)


def _src(name):
    src = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def _const(src, name):
    return int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))


# ---- the predictor against the header -----------------------------------------------------------------------------
def test_variant_table_equals_the_header():
    """kVariants / kNumVariants and the selection constants parsed out of sfl_engine.h equal the Python table: a
    variant added to the engine fails here until the sweep knows about it."""
    src = _src("sfl_engine.h")
    init = re.search(r"constexpr\s+WaveShape\s+kVariants\[\]\s*=\s*\{(.*?)\};", src, flags=re.S).group(1)
    rows = []
    for body in re.findall(r"\{([^{}]*)\}", init):
        f = [x.strip() for x in body.split(",")]
        assert len(f) in (5, 6), body  # PPL, SPL, TW, G, OCC (a number or a tuning macro) and, optionally, LM
        rows.append(tuple(int(x) for x in f[:4]) + (int(f[5]) if len(f) == 6 else 0,))
    assert tuple(rows) == sh.VARIANTS
    assert _const(src, "kNumVariants") == sh.NUM_VARIANTS == len(sh.VARIANTS)
    assert _const(src, "kFillWaves") == sh.FILL_WAVES
    assert _const(src, "kLmWaves") == sh.LM_WAVES
    assert _const(src, "kLmBytes") == sh.LM_BYTES
    assert int(re.search(r"#define\s+SFL_DEFAULT_G\s+(\d+)", src).group(1)) == sh.DEFAULT_G
    # the LDS words variant 11's kernel declares are the bytes the engine admits
    words = re.search(r"LM_WORDS\s*=\s*LM\s*\?\s*(\d+)\s*:\s*0", _src("sfl_wave.h")).group(1)
    assert int(words) * 4 == sh.LM_BYTES
    # every selection rule the predictor restates is still the header's: the three fits() terms, the default group
    # size, the small-batch rule and the LM rule
    sel = re.sub(r"\s+", "", src)
    for rule in ("md->S*4<=w.G*w.PPL&&md->S<=w.G*w.SPL&&md->T<=w.TW", "(md->T<=8?8:SFL_DEFAULT_G)",
                 "want_g<32&&n_envs*(uint64_t)want_g/64<kFillWaves)want_g=32",
                 "n_envs*(uint64_t)want_g/64<=kLmWaves&&lm_bytes(md)<=kLmBytes",
                 "returnhw*4*16+((int64_t)md->K*hw*4+1)/2*4"):
        assert rule in sel, rule


def test_predictor_on_the_stock_batches(monkeypatch):
    """The selections the engine's comments and the GPU suite state for the stock maps (tests/test_gpu.py,
    test_hparam_groups_gpu.py): c2 at 4,096 envs takes variant 11 (8 with SFL_LDS_MAP=0), at 65,536 variant 10; c3
    variant 7 from 16,384 envs on and 9 below; c5 variant 5; SFL_KERNEL=scalar the lane-per-env kernel."""
    for k in ("SFL_KERNEL", "SFL_WAVE_G", "SFL_LDS_MAP"):
        monkeypatch.delenv(k, raising=False)
    cms = {c: comp.compile_scenario(mapgen.make_config(c)) for c in ("c2", "c3", "c5")}

    def pick(cfg, E, **env):
        cm = cms[cfg]
        return sh.choose_variant(cm.S, cm.T, E, sh.lm_bytes(cm.H, cm.W, cm.K), env or None)

    assert sh.lm_bytes(cms["c2"].H, cms["c2"].W, cms["c2"].K) == 40_000 + 20_000
    assert [pick("c2", 4096), pick("c2", 4096, SFL_LDS_MAP="0"), pick("c2", 65536)] == [11, 8, 10]
    assert [pick("c3", 65536), pick("c3", 16384), pick("c3", 16383), pick("c5", 8)] == [7, 7, 9, 5]
    assert [pick("c2", 35, SFL_WAVE_G=g) for g in ("16", "32", "8", "64")] == [6, 11, 10, 1]
    assert [pick("c3", 28, SFL_WAVE_G=g) for g in ("16", "32", "8", "64")] == [7, 9, 2, 2]
    assert pick("c2", 4096, SFL_KERNEL="scalar") == 0
    monkeypatch.setenv("SFL_WAVE_G", "64")  # (env None: the process environment)
    assert pick("c2", 4096) == 1


# (row, expected variant at SFL_WAVE_G = 16 / 32 / 8 / 64), written from the limits of kVariants by hand
EXPECTED = {
    (5, 1, 8): (6, 11, 10, 1), (16, 8, 8): (6, 8, 10, 1), (16, 9, 8): (6, 8, 1, 1), (16, 16, 8): (6, 8, 1, 1),
    (16, 17, 8): (7, 8, 1, 1), (16, 32, 8): (7, 8, 1, 1), (16, 33, 8): (3, 3, 3, 3), (17, 8, 8): (7, 9, 2, 2),
    (17, 9, 8): (7, 9, 2, 2), (64, 31, 8): (7, 9, 2, 2), (64, 32, 8): (7, 9, 2, 2), (64, 33, 8): (3, 3, 3, 3),
    (65, 32, 8): (4, 4, 4, 4), (64, 64, 8): (3, 3, 3, 3), (64, 65, 8): (5, 5, 5, 5), (128, 64, 8): (4, 4, 4, 4),
    (129, 64, 8): (5, 5, 5, 5), (129, 9, 8): (5, 5, 5, 5), (128, 65, 8): (5, 5, 5, 5), (256, 127, 8): (5, 5, 5, 5),
    (255, 128, 8): (5, 5, 5, 5), (257, 64, 8): (0, 0, 0, 0), (16, 16, 3): (6, 11, 1, 1), (16, 32, 3): (7, 11, 1, 1), (16, 16, 4): (6, 8, 1, 1),
    (16, 32, 4): (7, 8, 1, 1), (16, 33, 3): (3, 3, 3, 3), (17, 9, 3): (7, 9, 2, 2),
}


@pytest.mark.parametrize("row", sh.ROWS, ids=lambda r: "%dx%dk%d" % r[:3])
def test_row_lands_on_the_expected_variant(row):
    cm = sh.compiled(row)
    lm = sh.lm_bytes(cm.H, cm.W, cm.K)
    if row[:3] in ((16, 16, 3), (16, 32, 3)):
        assert (cm.H, cm.W, lm) == (27, 27, 64_152) and sh.LM_BYTES - lm == 90 * 4
    if row[:3] in ((16, 16, 4), (16, 32, 4)):
        assert lm == 69_984
    got = tuple(sh.choose_variant(cm.S, cm.T, sh.n_envs(g), lm, {"SFL_WAVE_G": str(g)}) for g in (16, 32, 8, 64))
    assert got == EXPECTED[row[:3]]
    assert sh.wave64_variant(cm.S, cm.T) == got[3]


# ---- the coverage matrix, computed from the cases the GPU file runs -----------------------------------------------
# (variant: (the variant one switch past it, the variant one train past it)) at the same SFL_WAVE_G
NEXT = {1: (2, 3), 2: (4, 3), 3: (4, 5), 4: (5, 5), 5: (0, None), 6: (7, 7), 7: (4, 3), 8: (9, 3), 9: (4, 3),
        10: (2, 1), 11: (9, 3)}
# cells no case can reach, with the reason (at most 2)
EXEMPT = {(5, "one train past"): "sfl_create refuses a map of more than 128 trains: there is no kernel to launch",
          (5, "one switch past"): "257 switches leave every wave shape for the lane-per-env kernel, which "
                                  "test_gpu.py::test_fallback_kernel_is_reported runs; the predictor and the host "
                                  "build are still checked on the (257, 64) row here"}
NOT_ON_GPU = {(257, 64, 8, 4242)}


def _cells():
    return [(c, sh.predict(c)[0]) for c in sh.CASES]


def _lm(c):
    cm = sh.compiled(c.row)
    return sh.lm_bytes(cm.H, cm.W, cm.K)


def _lm_fits(c):
    return _lm(c) <= sh.LM_BYTES


def test_cases_are_distinct_and_sized_past_one_block():
    assert len(set(sh.CASES)) == len(sh.CASES) == len({sh.case_id(c) for c in sh.CASES})
    assert {c.row for c in sh.CASES} == set(sh.ROWS) - NOT_ON_GPU  # every other edge row runs on the GPU
    for g in (8, 16, 32, 64):
        per_block = 256 // g  # SFL_WAVE_BLOCK / SFL_GROUP_BLOCK threads
        assert sh.n_envs(g) > per_block and sh.n_envs(g) % per_block and sh.n_envs(g) <= sh.E_MAX


def test_every_variant_runs_every_instantiation():
    hit = {(v, c.mode) for c, v in _cells()}  # ("timed" here: an untruncated learn; truncation comes on top)
    missing = [(v, m) for v in WAVE for m in ("plain", "trace", "timed", "hpg") if (v, m) not in hit]
    assert not missing, missing
    part = {v for c, v in _cells() if c.mode == "part"}
    assert part == {1, 2, 3, 4, 5}, part  # k_wave_part<1..4> and k_wave2_part
    for v in (3, 4):  # both values of local_rows, on a full row and on one inside the envelope
        assert len({(c.row, c.arg) for c, u in _cells() if c.mode == "part" and u == v}) == 4
    fam = {("k_wave2" if v == 5 else "k_wave" if v < 5 else "two slots" if sh.VARIANTS[v][2] > sh.VARIANTS[v][3]
            else "one slot") for c, v in _cells() if c.mode == "trunc"}
    assert fam == {"k_wave", "k_wave2", "one slot", "two slots"}, fam


def test_every_variant_runs_on_and_one_past_each_limit():
    cells = [(c, v) for c, v in _cells() if c.mode != "part"]
    missing = []
    for v in WAVE:
        _, _, tw, g, lm = sh.VARIANTS[v]
        smax = sh.s_max(v)
        mine = [c for c, u in cells if u == v]
        if not any(c.row[1] == tw for c in mine):
            missing.append((v, "T == TW"))
        # (the generator builds every S asked for, so the binding row holds exactly s_max switches)
        took = max(c.row[0] for c in mine)
        print(f"variant {v}: T == TW = {tw}, largest S run {took} of {smax}")
        if took != smax:
            missing.append((v, "S binds"))
        # one past: the same group size asked for, the other limit still met, and for the LDS twins the same side of
        # the LDS limit -- so that only the limit in question sends the row elsewhere
        at_g = [(c, u) for c, u in cells if c.G == g and (v not in (8, 11) or _lm_fits(c) == bool(lm))]
        past_s = [u for c, u in at_g if c.row[0] == smax + 1 and c.row[1] <= tw]
        past_t = [u for c, u in at_g if c.row[1] == tw + 1 and c.row[0] <= smax]
        for name, got, want in (("one switch past", past_s, NEXT[v][0]), ("one train past", past_t, NEXT[v][1])):
            if (v, name) in EXEMPT:
                assert not got, f"{(v, name)} is reached: drop the exemption"
            elif want not in got:
                missing.append((v, name, got))
    # variant 11's third limit: a map that fits its registers and not its LDS takes variant 8, with nothing set
    if 8 not in [u for c, u in cells if c.G in (32, None) and sh.fits(11, *c.row[:2]) and not _lm_fits(c)]:
        missing.append((11, "just past the LDS limit"))
    if 11 not in [u for c, u in cells if sh.LM_BYTES - 512 <= _lm(c) <= sh.LM_BYTES]:
        missing.append((11, "just under the LDS limit"))
    assert not missing, missing
    assert len(EXEMPT) <= 2


# ---- the reference side of every GPU comparison: host build == oracle ---------------------------------------------
@pytest.mark.parametrize("row", sh.ROWS, ids=lambda r: "%dx%dk%d" % r[:3])
def test_host_build_equals_oracle(row):
    """Six envs stepped in chunks [50, 130] and through learn(2, exploit_freq=2): the host build's first and last env
    equal the oracle's Q dict, learn outputs and per-episode decisions; every grouped env of the rows the sweep runs
    with hyperparameter groups equals the oracle run with its group's hyperparameters."""
    from tests import hostsim
    runtime = sh.runtime
    cm, n = sh.compiled(row), 6
    b = sh.stepped(cm, sh.HP, sh.seeds(n), hostsim.lib())
    for e in (0, n - 1):
        assert b.q_dict(e) == sh.oracle_plain(row, sh.seeds(n)[e]), f"env {e}"
    # (envs are independent: the batch of 7 a one-env-per-wavefront case compares with holds the same 6)
    assert all(not sh.same_env(x, y) for x, y in zip(sh.snapshot(b, n), sh.host_plain(row, sh.CHUNKS, n + 1)))
    b.close()
    b = runtime.Batch(cm, sh.HP, sh.seeds(n), lib=hostsim.lib(), ntab=sh.NTAB)
    out = b.learn(sh.LEARN["n_episodes"], exploit_freq=sh.LEARN["exploit_freq"])
    ref = sh.oracle_learn(row, sh.seeds(n)[n - 1])
    assert not sh.learn_mismatches(out, n - 1, ref)
    assert b.q_dict(n - 1) == ref["q"]
    b.close()
    if any(c.row == row and c.mode == "hpg" for c in sh.CASES):
        b = sh.stepped(cm, sh.HANDLE_HP, sh.hpg_seeds(n), hostsim.lib(), hparam_groups=sh.GROUPS,
                       env_group=sh.env_groups(n))
        for e in (n - 2, n - 1):
            assert b.q_dict(e) == sh.oracle_plain(row, sh.hpg_seeds(n)[e], e % 2), f"env {e} (group {e % 2})"
        assert not np.array_equal(b.q_raw(0)[0], b.q_raw(1)[0])  # one seed, two groups: the tables differ
        b.close()


@pytest.mark.parametrize("case", [c for c in sh.CASES if c.mode == "trunc"], ids=sh.case_id)
def test_host_build_equals_oracle_truncating(case):
    """max_steps below the episode length: every learn episode of the oracle ends after max_steps + 1 decisions with
    trains still under way, and the host build agrees on every output."""
    from tests import hostsim
    cm, n = sh.compiled(case.row), 6
    b = sh.runtime.Batch(cm, sh.HP, sh.seeds(n), lib=hostsim.lib(), ntab=sh.NTAB, max_steps=case.arg)
    out = b.learn(sh.LEARN["n_episodes"], exploit_freq=sh.LEARN["exploit_freq"])
    for e in (0, n - 1):
        ref = sh.oracle_learn(case.row, sh.seeds(n)[e], case.arg)
        assert ref["decisions"] == [case.arg + 1] * sh.LEARN["n_episodes"]
        assert max(ref["out"]["arrived_trains"]) < cm.T
        assert not sh.learn_mismatches(out, e, ref)
        assert b.q_dict(e) == ref["q"]
    b.close()
