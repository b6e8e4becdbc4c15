"""Policy-bank evaluation on the MI355X (runtime.EvalBatch; cases and references: tests/_evalbank.py): the BANK
instantiation of every wave-kernel family and k_run's bank mode against the twin batch on the host build, bit for bit
-- per-env outputs, at_dest, the whole end state, the device-side fold against its numpy restatement computed from the
twin's outputs -- the read-only bank, truncation, the slot-epoch wrap over 258 launches, device-to-device copies from a
training batch, and the memory an evaluation handle does not allocate."""
import importlib
import subprocess
from collections import namedtuple

import numpy as np
import pytest

from tests import _evalbank as eb
from tests import _qfuzz as qf
from tests import _shapes as sh
from tests import hostsim

pytestmark = pytest.mark.gpu

runtime = sh.runtime
_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")

# one cell per kernel family, with tests/_qfuzz.py's cell settings; expect: (kernel_variant, group_lanes)
Cell = namedtuple("Cell", "name row G env expect", defaults=((), None))
CELLS = (
    Cell("g8", eb.row(16, 8), 8, expect=(10, 8)),
    Cell("g16", eb.row(16, 16), 16, expect=(6, 16)),
    Cell("v7", eb.row(16, 17), 16, expect=(7, 16)),                       # a translation unit's own scheduler elsewhere
    Cell("g32", eb.row(16, 32), 32, expect=(8, 32)),
    Cell("lm", eb.row(16, 16, 3), 32, expect=(11, 32)),                   # the map tables in LDS: a Bank cell of its own
    Cell("nolds", eb.row(16, 16, 3), 32, (("SFL_LDS_MAP", "0"),), (8, 32)),   # ... and its twin row on the same map
    Cell("g64", eb.row(16, 32), 64, expect=(1, 64)),
    Cell("ring", eb.row(16, 33), 64, expect=(3, 64)),                     # 33 trains: the two-slot ring
    Cell("wave2", eb.row(64, 65), 64, expect=(5, 64)),                    # k_wave2
    Cell("krun", eb.row(16, 17), None, (("SFL_KERNEL", "scalar"),), (0, 1)),
)
BY_NAME = {c.name: c for c in CELLS}


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


def _select(monkeypatch, cell):
    for k in ("SFL_KERNEL", "SFL_WAVE_G", "SFL_LDS_MAP", "SFL_REQUIRE_WAVE"):
        monkeypatch.delenv(k, raising=False)
    env = dict(cell.env)
    if cell.G is not None:
        env["SFL_WAVE_G"] = str(cell.G)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cm = sh.compiled(cell.row)
    n = sh.n_envs(cell.G)
    v = sh.choose_variant(cm.S, cm.T, n, sh.lm_bytes(cm.H, cm.W, cm.K), env)
    assert (v, sh.group_lanes(v)) == cell.expect, (cell.name, v)
    return n


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: c.name)
def test_twin_equality(lib, monkeypatch, cell):
    """Cases 1 - 3: e % 3 and then its permutation on one handle, each equal to its own twin in every output, the end
    state and the table (GPU cells equal the host build's: the restatement is computed from the twin's outputs)."""
    n = _select(monkeypatch, cell)
    eb.run_twin_equality(lib, cell.row, n, expect=cell.expect)


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: c.name)
def test_long_episodes(lib, monkeypatch, cell):
    """Case 3 on every cell: table (a) alone at max_steps = 100,000, terminated episodes whose trains are early, late and
    not arrived (all three non-zero: asserted on the twin, for every cell), so the fold's three classes are populated in
    every kernel family; at max_steps = 40 (test_twin_equality) they need not be."""
    n = _select(monkeypatch, cell)
    eb.run_long(lib, cell.row, n, expect=cell.expect)


@pytest.mark.parametrize("name", ["g8", "g64"])
def test_truncation(lib, monkeypatch, name):
    cell = BY_NAME[name]
    if name == "g64":
        cell = cell._replace(row=eb.row(16, 8))
    _select(monkeypatch, cell)
    eb.run_truncation(lib, eb.row(16, 8), 35)  # (35 envs: fewer leave no untruncated episode)


@pytest.mark.parametrize("G,expect", [(8, (10, 8)), (64, (1, 64))])
def test_epoch_wrap(lib, monkeypatch, G, expect):
    _select(monkeypatch, Cell("wrap", eb.row(5, 1), G, expect=expect))
    eb.run_epoch_wrap(lib, G)


def test_copy_policy(lib, monkeypatch):
    _select(monkeypatch, BY_NAME["g8"])
    eb.run_copy_policy(lib, eb.row(16, 8))


def test_gpu_cells_equal_host_cells(lib, monkeypatch):
    """The device fold against the host build's fold of the same evaluation, with more envs than a wavefront per policy
    and with every env on a policy of its own (the fold's two paths: the wave reduction and the lone lanes), and with
    env 7 alone on its policy in a wavefront whose other lanes share two (both paths in one wavefront: the lone lane is
    noted while the loop goes on and issues its atomics after it)."""
    cell = BY_NAME["g8"]
    _select(monkeypatch, cell)
    n = 200
    for P, pol in ((2, [0 if e % 5 else 1 for e in range(n)]), (n, list(range(n))),
                   (3, [2 if e == 7 else 0 if e % 5 else 1 for e in range(n)])):
        tabs = eb.tables(cell.row)
        cells = []
        for L in (lib, hostsim.lib()):
            ev = runtime.EvalBatch(sh.compiled(cell.row), sh.HP, qf.seeds(n), P, lib=L, max_steps=qf.MAX_STEPS)
            try:
                for p in range(P):
                    ev.set_policy_raw(p, *tabs[p % 3])
                cells.append(ev.evaluate(pol, per_env=False)["table"])
                if L is lib:
                    last, total = ev.fold_ms()
                    assert 0.0 < last <= total
            finally:
                ev.close()
        for k in _lib.EVAL_FIELDS:
            assert np.array_equal(cells[0][k], cells[1][k]), (P, k)
        assert cells[0]["episodes"].sum() == n


def test_no_per_env_q_block(lib, monkeypatch):
    """Case 8: an evaluation handle of 4,096 envs takes less than half of what the per-env Q blocks alone would."""
    import torch
    for k in ("SFL_KERNEL", "SFL_WAVE_G", "SFL_LDS_MAP", "SFL_REQUIRE_WAVE"):
        monkeypatch.delenv(k, raising=False)
    small = runtime.Batch(sh.compiled(eb.row(16, 8)), sh.HP, [1, 2], lib=lib, ntab=sh.NTAB)  # (the SeedSequence table exists now)
    small.close()
    cm = sh.compiled(eb.row(64, 32))
    n = 4096
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    ev = runtime.EvalBatch(cm, sh.HP, [300 + i for i in range(n)], 2, lib=lib, max_steps=qf.MAX_STEPS)
    try:
        after = torch.cuda.mem_get_info()[0]
        assert before - after < n * cm.q_per_env * 8 // 2, (before - after, n * cm.q_per_env * 8)
    finally:
        ev.close()


def test_both_libraries_export_the_entry_points(lib):
    names = ("sfl_create_eval", "sfl_bank_set", "sfl_bank_get", "sfl_bank_copy", "sfl_bank_eval", "sfl_bank_read",
             "sfl_bank_fold_ms")
    for path in (lib.path, hostsim.lib().path):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
        assert not [n for n in names if n not in exported], path
    assert lib.dll.sfl_abi_version() == 9
