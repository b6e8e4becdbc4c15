"""Seeded adversarial Q-tables through the fused kernels: the tables (``table``), the kernel cells and cases the GPU
sweep runs (tests/test_row_choice_gpu.py), the host-build references those cases compare with, and the oracle runs
with their hit counters that tests/test_row_choice.py compares the host build with.

A table is one env's compact Q block and key-set bitmap in Batch.q_raw's layout, drawn from
np.random.default_rng(SEED + env) and loaded with Batch.set_q_raw.  A row whose key-set bit is clear holds default_q
in every column, so the host build's q_dict of the loaded table is the whole table as the oracle's dict.

Two drivers: ``greedy`` loads the table and runs test(1) (F_GREEDY, nothing pending, nothing written); ``steps`` runs
learn_begin, apply_qinit, loads the table over the Q-init rows (they stay in the key set) and steps in two unequal
chunks.  max_steps = 40, as the truncation cases of tests/_shapes.py: an episode is cut after 41 decisions, so a
table whose STOP column always wins (stop_high) still ends its episodes."""
import functools
from collections import namedtuple

import numpy as np

from oracle import sfl_oracle as so
from tests import _shapes as sh
from tests import hostsim

runtime = sh.runtime

SEED = 77_000
MAX_STEPS = 40
CHUNKS = (30, 55)
# the stale cells' chunks: a staged row that an earlier decision of its batch wrote is rare (with sfl_wave.h pf_written
# cut to the row's first column, one env in 7 - 35 departs from the host build within 400 decisions, and on some
# cells none within 85), so these cells run longer and with three profiles
STALE_CHUNKS = (150, 250)
ZERO_SET = (0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308)
PROFILES = ("distinct", "ties", "stop_high", "stop_low", "zeros", "large")
TOUCH_P = dict(distinct=1.0, ties=0.5, stop_high=1.0, stop_low=1.0, zeros=0.5, large=0.5)  # P(a row is touched)

# hyperparameter sets of the steps driver (lr_decay_rate = 1 and ntab above the decision count: E_LR_TABLE cannot fire)
_BASE = dict(gamma=0.95, epsilon=0.0, epsilon_decay_rate=1.0, lr=0.2, lr_decay_rate=1.0, default_q=1.5)
HPS = dict(eps0=_BASE,                                            # every decision greedy, every post writes a cell
           eps1=dict(_BASE, epsilon=1.0),
           lr1=dict(_BASE, epsilon=0.3, lr=1.0, gamma=0.0),
           dq5=dict(_BASE, epsilon=0.3, lr=0.5, gamma=1.0, default_q=-5.0))
HPG_GROUPS = (HPS["eps0"], HPS["eps1"])                  # two interleaved groups, env e in group e % 2
HPG_HANDLE = dict(_BASE, epsilon=0.5, lr=0.25)           # matches neither


def hparams(profile, hp):
    """The hyperparameters of a case: ``hp`` names an entry of HPS ("greedy": the test driver, eps0's)."""
    h = dict(HPS["eps0" if hp in ("greedy", "hpg") else hp])
    if profile == "zeros":
        h["default_q"] = 0.0
    if profile == "large":  # |q| ~ 1e150: (1 - lr) q + lr (r + gamma max) stays far below overflow
        h.update(gamma=1.0, lr=0.5)
    return h


# ---- the tables -----------------------------------------------------------------------------------------------------
def table(cm, profile, default_q, env, keep=None):
    """(Q block, key-set words) of env ``env``; ``keep``: key-set words that stay set (the Q-init rows)."""
    rng = np.random.default_rng(SEED + env)
    A = cm.arrays
    q = np.full(cm.q_per_env, float(default_q))
    t = np.zeros((cm.rows_per_env + 31) // 32, np.uint32) if keep is None else keep.copy()
    dq = float(default_q)
    for s in range(cm.S):
        for slot in range(len(cm.ports[s])):
            g = 4 * s + slot
            n, w = (1 << len(cm.ports[s])) * cm.K * 3, int(A["q_w"][g])
            on = rng.random(n) < TOUCH_P[profile]
            if profile in ("distinct", "stop_high", "stop_low"):
                v = rng.standard_normal((n, w)) * 100.0
                if profile != "distinct":
                    v[:, w - 1] = dq + (1000.0 if profile == "stop_high" else -1000.0)
            elif profile == "ties":
                v = rng.choice([dq - 1.0, dq, dq + 1.0], (n, w))
            elif profile == "zeros":
                v = rng.choice(ZERO_SET, (n, w))
            else:
                v = rng.choice([-1.0, 1.0], (n, w)) * rng.uniform(0.5, 2.0, (n, w)) * 1e150
            v[~on] = dq
            off = int(A["q_off"][g])
            q[off: off + n * w] = v.reshape(-1)
            rid = int(A["row_base"][g]) + np.nonzero(on)[0]
            np.bitwise_or.at(t, rid >> 5, (np.uint32(1) << (rid & 31).astype(np.uint32)))
    return q, t


def load(b, profile, n, over_qinit):
    dq = b.hp["default_q"]
    for e in range(n):
        keep = b.q_raw(e)[1] if over_qinit else None
        b.set_q_raw(e, *table(b.cm, profile, dq, e, keep))


def run(b, profile, hp, n, chunks=CHUNKS):
    """A case's driver on a batch of n envs; returns test(1)'s outputs (greedy) or None."""
    if hp == "greedy":
        load(b, profile, n, False)
        return b.test(1)
    b.learn_begin()
    b.apply_qinit()
    load(b, profile, n, True)
    for k in chunks:
        got, _ = b.step(k)
        assert got == k * n
    return None


# ---- kernel cells and cases -------------------------------------------------------------------------------------------
# env: further kernel-selection settings; chunks: the steps driver's; stale: a cell meant for the stale-staging hazard
Cell = namedtuple("Cell", "name row G env hpg chunks stale", defaults=((), False, CHUNKS, False))


def _row(S, T, K=8):
    r = [r for r in sh.ROWS if r[:3] == (S, T, K)]
    assert len(r) == 1
    return r[0]


def _one_station(S, T):
    """A scenario of tests/_shapes.py's generator with one station: every train has the same target, so two trains
    meet on one Q row far more often (the oracle reaches the stale-staging hazard 0 - 2 times in 8 envs on the rows of
    _shapes.ROWS with 8 stations, 1 - 4 times per env here)."""
    key = ("one-station", S, T, 1, 4242)
    sh.DERIVED[key] = lambda: sh.mapgen.generate(S, T, 1, seed=4242, malfunction=(0.01, 5, 15), name="edge")
    return key


CELLS = (
    Cell("g8", _row(16, 8), 8),
    Cell("g16", _row(16, 16), 16),
    Cell("g32", _row(16, 32), 32),
    Cell("g64", _row(16, 32), 64),
    Cell("ring", _row(16, 33), 64),                         # the two-slot ring shape (33 - 128 trains): k_wave2
    Cell("v7", _row(16, 17), 16),                           # variant 7: a translation unit of its own
    Cell("nolds", _row(16, 16, 3), 32, (("SFL_LDS_MAP", "0"),)),   # variant 11's map without its LDS tables
    Cell("hpg16", _row(16, 16), 16, hpg=True),
    Cell("hpg64", _row(16, 32), 64, hpg=True),
    Cell("krun", _row(16, 17), None, (("SFL_KERNEL", "scalar"),)),  # the lane-per-env kernel, every profile
    Cell("krun257", _row(257, 64), None),                   # ... on a map one switch past every wave shape
    # two trains of one env on one row in one tick (instrument's ``stale``), per kernel family that stages rows
    Cell("s-g8", _one_station(16, 8), 8, chunks=STALE_CHUNKS, stale=True),
    Cell("s-g16", _one_station(16, 16), 16, chunks=STALE_CHUNKS, stale=True),
    Cell("s-v7", _one_station(16, 17), 16, chunks=STALE_CHUNKS, stale=True),
    Cell("s-g32lm", _one_station(16, 16), 32, chunks=STALE_CHUNKS, stale=True),  # variant 11: the map tables in LDS
    Cell("s-g64", _one_station(16, 16), 64, chunks=STALE_CHUNKS, stale=True),
    Cell("s-ring", _one_station(16, 36), 64, chunks=STALE_CHUNKS, stale=True),
)
FULL = ("g16", "ring", "krun")  # every profile runs here
EXPECT = {"g8": (10, 8), "g16": (6, 16), "g32": (8, 32), "g64": (1, 64), "ring": (3, 64), "v7": (7, 16), "nolds": (8, 32),
          "hpg16": (6, 16), "hpg64": (1, 64), "krun": (0, 1), "krun257": (0, 1), "s-g8": (10, 8), "s-g16": (6, 16),
          "s-v7": (7, 16), "s-g32lm": (11, 32), "s-g64": (1, 64), "s-ring": (3, 64)}  # (kernel_variant, group_lanes)

Case = namedtuple("Case", "cell profile hp")


def _cases():
    out = []
    for c in CELLS:
        if c.hpg:
            out += [Case(c, p, "hpg") for p in ("ties", "distinct")]
        elif c.stale:
            out += [Case(c, p, "eps0") for p in ("ties", "distinct", "large")]
        elif c.name in FULL:
            out += [Case(c, p, hp) for p in PROFILES for hp in ("greedy", "eps0")]
            out += [Case(c, "ties", hp) for hp in ("eps1", "lr1", "dq5")]
        elif c.name == "krun257":  # (920,064 Q cells per env: the two cases every cell runs)
            out += [Case(c, "ties", "greedy"), Case(c, "ties", "eps0")]
        else:
            out += [Case(c, "ties", "greedy"), Case(c, "ties", "eps0"), Case(c, "zeros", "eps0")]
    return tuple(out)


CASES = _cases()


def case_id(c):
    return f"{c.cell.name}-{c.profile}-{c.hp}"


def cell_env(cell):
    env = dict(cell.env)
    if cell.G is not None:
        env["SFL_WAVE_G"] = str(cell.G)
    return env


def predict(cell):
    """(kernel_variant, group_lanes) by tests/_shapes.py's restatement of choose_variant."""
    cm = sh.compiled(cell.row)
    v = sh.choose_variant(cm.S, cm.T, n_envs(cell), sh.lm_bytes(cm.H, cm.W, cm.K), cell_env(cell))
    return v, sh.group_lanes(v)


def n_envs(cell):
    return sh.n_envs(cell.G)


def seeds(n):
    return [300 + i for i in range(n)]


def hpg_seeds(n):
    return [300 + i // 2 for i in range(n)]


def row_chunks(row):
    ch = {c.chunks for c in CELLS if c.row == row}
    assert len(ch) == 1
    return ch.pop()


def _n_row(row, hpg):
    return max(n_envs(c) for c in CELLS if c.row == row and c.hpg == hpg)


def oracle_envs(row, hpg):
    """The envs the CPU file compares with the oracle: the first and the last three of every cell of the row (the 257
    switches of k_run's: the first and the last; a stale cell: every env, since the hazard is met by few of them)."""
    out = set()
    for c in CELLS:
        if c.row == row and c.hpg == hpg:
            n = n_envs(c)
            out |= set(range(n)) if c.stale else {0, n - 1} if c.name == "krun257" else {0, 1, 2, n - 3, n - 2, n - 1}
    return sorted(out)


# ---- references: the host build, once per (row, profile, hp) -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host(row, profile, hp):
    """(snapshot of every env after the run, test outputs or None, {env: (Q block, key set)} of the loaded tables of
    the oracle envs) of the host build on the most envs a cell of the row runs."""
    hpg = hp == "hpg"
    n = _n_row(row, hpg)
    kw = dict(hparam_groups=HPG_GROUPS, env_group=[e % 2 for e in range(n)]) if hpg else {}
    b = runtime.Batch(sh.compiled(row), HPG_HANDLE if hpg else hparams(profile, hp), hpg_seeds(n) if hpg else seeds(n),
                      lib=hostsim.lib(), ntab=sh.NTAB, max_steps=MAX_STEPS, **kw)
    over = hp != "greedy"
    if over:
        b.learn_begin()
        b.apply_qinit()
    load(b, profile, n, over)
    loaded = {e: b.q_raw(e) for e in oracle_envs(row, hpg)}
    if over:
        for k in row_chunks(row):
            got, _ = b.step(k)
            assert got == k * n
    out = None if over else b.test(1)
    snap = sh.snapshot(b, n)
    b.close()
    return snap, out, loaded


class _Rows:
    """Stored (Q block, key set) pairs read as runtime.Batch.q_dict reads a batch's."""
    q_dict = runtime.Batch.q_dict

    def __init__(self, cm, default_q, raw):
        self.cm, self.hp, self.raw = cm, dict(default_q=default_q), raw

    def q_raw(self, e):
        return self.raw[e]


def q_dicts(row, profile, hp):
    """({env: Q dict of the loaded table}, {env: Q dict after the run}) of the host build, for the oracle envs."""
    snap, _, loaded = host(row, profile, hp)
    dq = (HPG_HANDLE if hp == "hpg" else hparams(profile, hp))["default_q"]
    before, after = _Rows(sh.compiled(row), dq, loaded), _Rows(sh.compiled(row), dq, {e: snap[e][:2] for e in loaded})
    return {e: before.q_dict(e) for e in loaded}, {e: after.q_dict(e) for e in loaded}


def same_bits(x, y):
    """Equal as bit patterns: float64 arrays are compared as uint64 (-0.0 and +0.0 differ), others as they are."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if x.dtype == np.float64 and y.dtype == np.float64:
        x, y = x.view(np.uint64), y.view(np.uint64)
    return x.dtype == y.dtype and np.array_equal(x, y)


def same_env_bits(got, ref):
    """tests/_shapes.py same_env with the Q-table compared as bit patterns: the mismatching parts of two snapshot
    entries (empty: bit-equal)."""
    bad = [] if same_bits(got[0], ref[0]) else ["Q-table bits"]
    return bad + sh.same_env(got, ref)


def dict_bits(d):
    """A Q dict with its values as bit patterns (-0.0 and +0.0 differ)."""
    return {k: np.array(v, np.float64).view(np.uint64).tolist() for k, v in d.items()}


# ---- the oracle with hit counters --------------------------------------------------------------------------------------
HITS = ("forbidden", "filler_wins", "tie_filler_low", "tie_filler_high", "stale", "truncated")


def _stored(cm, sidx, key):
    """The full-row actions a row stores (its in-port's routes and STOP)."""
    s = sidx[(key[0], key[1])]
    P = len(cm.ports[s])
    dl = key[2 + 3 * P: 2 + 4 * P]
    slot = [i for i in range(P) if dl[i] != -1]
    assert len(slot) == 1
    return {a for a, (src, _) in enumerate(cm.outcomes[s]) if src == slot[0]} | {int(cm.n_actions[s]) - 1}


def instrument(model, cm, loaded, over_init):
    """Count on the oracle, by wrapping max_action / update / on_step and the env's step / reset (never on the code
    under test):
    forbidden: greedy decisions whose unmasked argmax the mask forbids (the ``arg`` fallback);
    filler_wins: ... whose unmasked argmax is a filler action;
    tie_filler_low / _high: ... of a row that is not constant, whose maximum is shared by a stored column and the
        filler, the first filler index below / above the first such stored column;
    stale: greedy decisions on a row that another train's update wrote earlier in the same tick of the same episode
        (the stale-staging hazard); the writer of a pending update is the train whose decision posted it, the writer
        of an arrival bonus an arrived train, which decides no more;
    truncated: episodes cut by max_steps."""
    hits = dict.fromkeys(HITS, 0)
    env = model.env
    sidx = {sid: i for i, sid in enumerate(cm.switch_ids)}
    inner_ma, inner_up, inner_init = model.max_action, model.update, model.init_q_table
    inner_step, inner_reset = env.step, env.reset
    cur = dict(h=None)  # the train of the decision being stepped
    written = {}        # row -> (tick, writer) of its last write in this episode (ticks restart at every reset)

    def max_action(state, agent, mask):
        key = tuple(int(x) for x in state)
        row = list(model._row(state, agent))
        stored = _stored(cm, sidx, key)
        best = int(np.argmax(row))
        hits["forbidden"] += 0 if mask[best] else 1
        hits["filler_wins"] += 0 if best in stored else 1
        top = [a for a in range(len(row)) if row[a] == row[best]]
        ts, tf = [a for a in top if a in stored], [a for a in top if a not in stored]
        if ts and tf and len(set(row)) > 1:
            hits["tie_filler_low" if tf[0] < ts[0] else "tie_filler_high"] += 1
        w = written.get(key)
        if w is not None and w[0] == env.now() and w[1] != env.active_train:
            hits["stale"] += 1
        return inner_ma(state, agent, mask)

    def step(action):
        cur["h"] = env.active_train  # (greedy or exploratory: the train that decides, before the step moves on)
        return inner_step(action)

    def reset(*a, **kw):
        written.clear()
        return inner_reset(*a, **kw)

    def update(state, action, reward, next_state, *a):
        inner_up(state, action, reward, next_state, *a)
        written[tuple(int(x) for x in state)] = (env.now(), None if next_state is None else cur["h"])

    def init_q_table():
        inner_init()
        model.q.update({k: list(v) for k, v in loaded.items()})

    def on_step(e, *a):
        if e.truncated and not e.terminated:
            hits["truncated"] += 1

    model.max_action, model.update, model.on_step = max_action, update, on_step
    env.step, env.reset = step, reset
    if over_init:
        model.init_q_table = init_q_table
    else:
        model.q = {k: list(v) for k, v in loaded.items()}
    return hits


@functools.lru_cache(maxsize=None)
def _loaded(row, profile, hp):
    return q_dicts(row, profile, hp)[0]


@functools.lru_cache(maxsize=None)
def oracle(row, profile, hp, env):
    """(Q dict, test outputs or None, hit counts) of the oracle on env ``env``'s loaded table."""
    hpg = hp == "hpg"
    loaded = _loaded(row, profile, hp)
    h = dict(HPG_GROUPS[env % 2], gamma=HPG_HANDLE["gamma"], default_q=HPG_HANDLE["default_q"]) if hpg \
        else hparams(profile, hp)
    seed = (hpg_seeds if hpg else seeds)(env + 1)[env]
    _, model = so.build(sh.scenario(row), seed, h, max_steps=MAX_STEPS, trace=False)
    hits = instrument(model, sh.compiled(row), loaded[env], hp != "greedy")
    out = None
    if hp == "greedy":
        out = model.test()
    else:
        so.run_decisions(model, sum(row_chunks(row)))
    return model.q, out, hits
