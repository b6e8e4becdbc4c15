"""Step-mode learning curves (include/sfl.h sfl_curve_*): the cases, a numpy model of the fold and the checks that
tests/test_curve.py runs on the host build and tests/test_curve_gpu.py on the MI355X.

The reference is never the code under test: the host build's learn(N) per-episode, per-env records (pinned to the oracle
and the goldens by the parity tests) are binned here with the rule of include/sfl.h.  learn(N) and learn_begin,
apply_qinit, step(a), step(b), ... walk the same trajectory, so a launch that brings an env to D decisions in total has
ended exactly the episodes whose decisions sum to less than D (an episode whose last decision is the launch's last is
ended by the next launch): ``expected_marks`` derives every env's episode count after every chunk from the records'
``decisions``, the checks assert that ``curve()["episodes"]`` equals it, and the model folds from there."""
import functools
import warnings
from collections import namedtuple

import numpy as np

from tests import _shapes as sh
from tests import hostsim

_lib = sh.runtime._lib
FIELDS = _lib.CURVE_FIELDS
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min

# row: a tests/_shapes.ROWS map as (S, T); G: SFL_WAVE_G ("scalar": SFL_KERNEL=scalar, None: unset); E: envs (None:
# 256 / G + 3); series: None (one series), ("mod", k) for env_series = e % k, ("lone", k) for env 0 alone on series
# k - 1 and every other env on e % (k - 1), "hpg" for a grouped handle with NULL series
# seed0: the envs run the seeds from seed0 upward (tests/_shapes.seeds starts at 300 too), STUCK left out
Case = namedtuple("Case", "name row G max_steps chunks bin_episodes n_bins ring series E seed0",
                  defaults=(None, None, 300))


def _row(S, T):
    row = [r for r in sh.ROWS if r[:3] == (S, T, 8)]
    assert len(row) == 1
    return row[0]


MIXED = Case("mixed", _row(16, 8), 8, 60, (150, 250), 2, 4, 256)
FAMILIES = tuple(Case(f"families-{S}x{T}-{G}", _row(S, T), G, 40, (150, 250), 2, 3, 256)
                 for S, T, G in ((16, 16, 16), (16, 16, 32), (16, 16, 64), (16, 17, 16), (16, 33, 64), (16, 8, 8),
                                 (16, 16, "scalar")))
SERIES = (Case("series-mod3", _row(16, 16), 16, 40, (150, 250), 2, 3, 256, ("mod", 3)),
          Case("series-hpg", _row(16, 16), 16, 40, (150, 250), 2, 3, 256, "hpg"))
# (seed 308 circles the 5x1 map for 10 decisions an episode and ends only 14 episodes in the case's 120 decisions: the
# case's 19 envs start one seed later, where every env ends more than ring = 16 -- check_reference asserts it)
SHORT = Case("short", _row(5, 1), 16, 100_000, (15,) * 8, 8, 4, 16, seed0=309)
LOST = Case("lost", _row(5, 1), 16, 100_000, (30, 55), 8, 4, 2)
EDGES = tuple(Case(f"edges-{E}", _row(5, 1), None, 100_000, (15, 15), 4, 3, 16, ("mod", 5), E)
              for E in (1, 63, 64, 65, 257))
# env 0 alone on its series beside four series of 16 envs each in wavefront 0 (a lone lane and shared cells in one
# wavefront: the fold notes the lone lane, goes on reducing the others and lets it issue its atomics after the loop);
# env 64 is the only lane of wavefront 1
LONE = Case("lone-65", _row(5, 1), None, 100_000, (15, 15), 4, 3, 16, ("lone", 5), 65)
CASES = (MIXED,) + FAMILIES + SERIES + (SHORT, LOST) + EDGES + (LONE,)
UNCHANGED = (Case("unchanged-16x16", _row(16, 16), 16, 40, (150, 250), 2, 3, 8, ("mod", 3)),
             Case("unchanged-5x1", _row(5, 1), 16, 100_000, (30, 55), 8, 4, 2))


def n_envs(c):
    return c.E if c.E is not None else sh.n_envs(c.G if isinstance(c.G, int) else 16)


# Seeds below 700 with which the 5x1 map's one train is broken down from its departure to the end of the timetable in
# every episode: such an env makes no decision, its learn() records say decisions == 0, and no decision budget ever
# ends its sfl_step.  No case runs them (records() asserts that every env decides in its first episode).
STUCK = frozenset((346, 353, 359, 430, 451, 557, 582, 596, 602, 609, 617))


def seeds_of(c):
    n = n_envs(c)
    if c.series == "hpg":
        return tuple(sh.hpg_seeds(n))
    assert c.seed0 + n + len(STUCK) < 700
    return tuple(s for s in range(c.seed0, 700) if s not in STUCK)[:n]


def case_env(c):
    """The kernel-selection settings a case runs under (everything else unset)."""
    if c.G == "scalar":
        return {"SFL_KERNEL": "scalar"}
    return {} if c.G is None else {"SFL_WAVE_G": str(c.G)}


def predict(c):
    """(kernel_variant, group_lanes) a device handle of the case must report."""
    cm = sh.compiled(c.row)
    v = sh.choose_variant(cm.S, cm.T, n_envs(c), sh.lm_bytes(cm.H, cm.W, cm.K), case_env(c))
    return v, sh.group_lanes(v)


def series_of(c):
    n = n_envs(c)
    if c.series is None:
        return None, 1
    if c.series == "hpg":
        return np.array(sh.env_groups(n)), len(sh.GROUPS)
    kind, k = c.series
    if kind == "lone":
        ser = np.arange(n) % (k - 1)
        ser[0] = k - 1
        return ser, k
    return np.arange(n) % k, k


def make_batch(c, lib, curve=True, **kw):
    """The case's batch on ``lib`` after learn_begin and apply_qinit, with the case's curve unless ``curve`` is False."""
    n = n_envs(c)
    case_records(c)  # (refuses seeds that never decide before anything steps them)
    if c.series == "hpg":
        b = sh.runtime.Batch(sh.compiled(c.row), sh.HANDLE_HP, seeds_of(c), lib=lib, ntab=sh.NTAB,
                             max_steps=c.max_steps, hparam_groups=sh.GROUPS, env_group=sh.env_groups(n), **kw)
    else:
        b = sh.runtime.Batch(sh.compiled(c.row), sh.HP, seeds_of(c), lib=lib, ntab=sh.NTAB, max_steps=c.max_steps, **kw)
    b.learn_begin()
    b.apply_qinit()
    if curve:
        ser, ns = series_of(c)
        explicit = None if c.series in (None, "hpg") else ser
        assert b.curve_begin(c.bin_episodes, c.n_bins, explicit, ns, c.ring) == c.ring
    return b


# ---- the reference: learn(N) on the host build, once per (map, hyperparameters, envs) -------------------------------
@functools.lru_cache(maxsize=None)
def _host_learn(row, max_steps, seeds, hpg, n_episodes):
    if hpg:
        b = sh.runtime.Batch(sh.compiled(row), sh.HANDLE_HP, seeds, lib=hostsim.lib(), ntab=sh.NTAB,
                             max_steps=max_steps, hparam_groups=sh.GROUPS, env_group=sh.env_groups(len(seeds)))
    else:
        b = sh.runtime.Batch(sh.compiled(row), sh.HP, seeds, lib=hostsim.lib(), ntab=sh.NTAB, max_steps=max_steps)
    out = b.learn(n_episodes)
    b.close()
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def records(row, max_steps, seeds, hpg, decisions, skip=0):
    """The host build's learn(N) records with N large enough that every env's episodes from ``skip`` on make
    ``decisions`` decisions or more (so N is at least the number of episodes any env ends within them)."""
    n_ep = 16
    while True:
        out = _host_learn(row, max_steps, seeds, hpg, n_ep)
        assert out["decisions"][0].min() > 0, "an env that never decides: sfl_step would not return"
        if out["decisions"][skip:].sum(axis=0).min() >= decisions:
            return out
        n_ep *= 2


def case_records(c):
    return records(c.row, c.max_steps, seeds_of(c), c.series == "hpg", sum(c.chunks))


def expected_marks(rec, chunks, start=0):
    """Each env's episode index after each chunk, for envs that stood at the start of episode ``start``."""
    cum = np.cumsum(rec["decisions"][start:].astype(np.int64), axis=0)
    marks, total = [], 0
    for d in chunks:
        total += d
        assert (cum[-1] >= total).all()
        marks.append(start + (cum < total).sum(axis=0))
    return marks


def empty_cells(n_bins, n_series):
    cells = {k: np.zeros((n_bins, n_series), np.int64) for k in FIELDS}
    for k in ("arrived_min", "reward_min", "first_episode"):
        cells[k][:] = I64_MAX
    for k in ("arrived_max", "reward_max"):
        cells[k][:] = I64_MIN
    cells["last_episode"][:] = -1
    return cells


def model(rec, marks, series, n_series, bin_episodes, n_bins, ring, T, max_steps, start=0):
    """The fold of include/sfl.h, one launch, one env, one episode at a time: ``marks[k][e]`` is env e's episode index
    after launch k.  Returns (cells, episodes kept per launch [launch][env])."""
    cells = empty_cells(n_bins, n_series)
    E = len(marks[0])
    series = np.zeros(E, np.int64) if series is None else series
    mark = np.full(E, start, np.int64)
    kept = np.zeros((len(marks), E), np.int64)
    for k, now in enumerate(marks):
        for e in range(E):
            a, b, s = int(now[e]), int(mark[e]), int(series[e])
            first = max(b, a - ring)
            for i in range(b, a):
                cell = (min(i // bin_episodes, n_bins - 1), s)
                if i < first:
                    cells["lost"][cell] += 1
                    continue
                kept[k, e] += 1
                arrived, reward = int(rec["arrived"][i, e]), float(rec["cum_reward"][i, e])
                assert reward == int(reward)
                reward, dec = int(reward), int(rec["decisions"][i, e])
                cells["count"][cell] += 1
                cells["arrived_sum"][cell] += arrived
                cells["arrived_min"][cell] = min(cells["arrived_min"][cell], arrived)
                cells["arrived_max"][cell] = max(cells["arrived_max"][cell], arrived)
                cells["all_arrived"][cell] += arrived == T
                cells["reward_sum"][cell] += reward
                cells["reward_min"][cell] = min(cells["reward_min"][cell], reward)
                cells["reward_max"][cell] = max(cells["reward_max"][cell], reward)
                cells["decisions_sum"][cell] += dec
                cells["ticks_sum"][cell] += int(rec["ticks"][i, e])
                cells["malfunctions_sum"][cell] += int(rec["num_malfunctions"][i, e])
                cells["delay_sum"][cell] += int(rec["delays"][i, :, e].sum())
                cells["truncated"][cell] += dec > max_steps
                cells["first_episode"][cell] = min(cells["first_episode"][cell], i)
                cells["last_episode"][cell] = max(cells["last_episode"][cell], i)
        mark = np.asarray(now, np.int64)
    return cells, kept


def assert_cells(got, want, what=""):
    for k in FIELDS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), f"{what}{k}:\n{got[k]}\nmodel:\n{want[k]}"


def assert_means(cv):
    """The derived float means of Batch.curve() restate the integer fields, NaN where no episode was folded."""
    cnt = cv["count"]
    for k, num in (("arrived_mean", "arrived_sum"), ("reward_mean", "reward_sum"), ("decisions_per_episode", "decisions_sum"),
                   ("truncated_frac", "truncated"), ("all_arrived_frac", "all_arrived")):
        assert np.isnan(cv[k][cnt == 0]).all() and np.array_equal(cv[k][cnt > 0], cv[num][cnt > 0] / cnt[cnt > 0]), k
    assert np.isnan(cv["ticks_per_decision"][cnt == 0]).all()
    assert np.array_equal(cv["ticks_per_decision"][cnt > 0], cv["ticks_sum"][cnt > 0] / cv["decisions_sum"][cnt > 0])


# ---- what each case claims about its reference, asserted on the learn() records -------------------------------------
def check_reference(c, rec, marks, kept, want):
    n, T = n_envs(c), sh.compiled(c.row).T
    done = int(max(marks[-1]))
    dec, arr = rec["decisions"][:done, :n], rec["arrived"][:done, :n]
    ended = np.arange(done)[:, None] < marks[-1][None, :]  # the episodes the case folds or loses
    if c.name == "mixed":
        trunc = dec > c.max_steps
        assert (trunc & ended).any() and (~trunc & ended).any()
        assert len(set(arr[ended].tolist())) >= 3 and (arr[ended] == T).any()
        assert want["delay_sum"].sum() != 0 and want["malfunctions_sum"].sum() != 0
    if c.name.startswith("families") or c.name.startswith("series"):
        assert (dec[ended] == c.max_steps + 1).any()  # truncated episodes: max_steps + 1 decisions
        assert c.row[:2] != (16, 16) or ((dec[ended] == c.max_steps + 1).all() and 1 <= arr[ended].min() < arr[ended].max())
        assert (marks[-1] - c.bin_episodes * (c.n_bins - 1) >= 2).all()  # two or more episodes clamped into the last bin
    if c.name.startswith("series"):
        assert not all(np.array_equal(want[k][:, 0], want[k][:, 1]) for k in FIELDS)
    if c.name == "short":
        assert want["lost"].sum() == 0 and max(c.chunks) + 1 <= c.ring
        assert (marks[-1] > c.ring).all()  # the ring has wrapped for every env
    if c.name == "lost":
        assert (want["lost"].sum(axis=1) > 0).sum() >= 2 and (kept == c.ring).all()
    if c.name.startswith("edges"):
        assert want["count"].sum() > 0 and (n < 5 or (want["count"].sum(axis=0) > 0).all())
    if c.name.startswith("lone"):
        ser = series_of(c)[0]
        assert (ser == c.series[1] - 1).sum() == 1 and np.bincount(ser[:64])[:-1].min() >= 2  # alone beside shared series
        assert want["count"][:, c.series[1] - 1].sum() > 0


def step(b, c, d):
    """b.step(d); the once-only warning of a ring below d + 1 rows is what the lost / unchanged cases are about."""
    with warnings.catch_warnings():
        if c.ring < d + 1:
            warnings.simplefilter("ignore", RuntimeWarning)
        return b.step(d)[0]


def run_case(c, lib, check_kernel=False):
    """The case on ``lib``: episodes after every chunk and every field of every cell against the model."""
    n, cm = n_envs(c), sh.compiled(c.row)
    rec = case_records(c)
    marks = expected_marks(rec, c.chunks)
    ser, ns = series_of(c)
    want, kept = model(rec, marks, ser, ns, c.bin_episodes, c.n_bins, c.ring, cm.T, c.max_steps)
    check_reference(c, rec, marks, kept, want)
    b = make_batch(c, lib)
    if check_kernel:
        cnt = b.counters()
        assert (cnt["kernel_variant"], cnt["group_lanes"]) == predict(c), (cnt, predict(c))
    for k, d in enumerate(c.chunks):
        assert step(b, c, d) == d * n
        assert np.array_equal(b.curve()["episodes"], marks[k]), f"episodes after chunk {k}"
    cv = b.curve()
    assert_cells(cv, want)
    assert_means(cv)
    srs = np.zeros(n, np.int64) if ser is None else ser
    for s in range(ns):
        assert (cv["count"][:, s] + cv["lost"][:, s]).sum() == cv["episodes"][srs == s].sum()
    b.close()


def run_unchanged(c, lib):
    """Recording must not perturb training: a batch with a curve and a twin without one end bit-equal."""
    n = n_envs(c)
    with_curve, twin = make_batch(c, lib), make_batch(c, lib, curve=False)
    for d in c.chunks:
        assert step(with_curve, c, d) == twin.step(d)[0] == d * n
    assert with_curve.curve()["count"].sum() > 0
    for e, (got, want) in enumerate(zip(sh.snapshot(with_curve, n), sh.snapshot(twin, n))):
        assert not sh.same_env(got, want), f"env {e}: {sh.same_env(got, want)}"
    with_curve.close()
    twin.close()


# ---- lifecycle -------------------------------------------------------------------------------------------------------
LIFE = Case("lifecycle", _row(5, 1), 16, 100_000, (15, 15), 4, 3, 16, ("mod", 5))


def run_learn_begin_resets(lib):
    c = LIFE
    b = make_batch(c, lib)
    for d in c.chunks:
        b.step(d)
    assert b.curve()["count"].sum() > 0 and b.curve()["episodes"].min() > 0
    b.learn_begin()
    cv = b.curve()
    assert_cells(cv, empty_cells(c.n_bins, series_of(c)[1]), "after learn_begin: ")
    assert not cv["episodes"].any()
    b.close()


def run_learn_leaves_curve(lib):
    """learn(2) on a handle with a curve: the same arrays as a twin without one, the cells untouched, the marks at the
    envs' episode indices -- the steps that follow fold their own episodes only."""
    c = LIFE
    n, cm = n_envs(c), sh.compiled(c.row)
    b, twin = make_batch(c, lib), make_batch(c, lib, curve=False)
    out, ref = b.learn(2), twin.learn(2)
    for k in ref:
        assert np.array_equal(out[k], ref[k]), k
    cv = b.curve()
    assert_cells(cv, empty_cells(c.n_bins, series_of(c)[1]), "after learn(2): ")
    assert (cv["episodes"] == 2).all()
    rec = records(c.row, c.max_steps, seeds_of(c), False, sum(c.chunks), 2)
    for k in ref:
        assert np.array_equal(rec[k][:2], ref[k]), k  # (learn(2) is the start of the reference's learn(N))
    marks = expected_marks(rec, c.chunks, 2)
    ser, ns = series_of(c)
    want, _ = model(rec, marks, ser, ns, c.bin_episodes, c.n_bins, c.ring, cm.T, c.max_steps, 2)
    for k, d in enumerate(c.chunks):
        b.step(d)
        assert np.array_equal(b.curve()["episodes"], marks[k])
    assert want["count"].sum() > 0 and want["first_episode"].min() == 2
    assert_cells(b.curve(), want)
    b.close()
    twin.close()


def run_curve_end(lib):
    c = LIFE
    n = n_envs(c)
    b, twin = make_batch(c, lib), make_batch(c, lib, curve=False)
    b.step(c.chunks[0])
    twin.step(c.chunks[0])
    b.curve_end()
    for call in (b.curve, b.curve_end):
        try:
            call()
        except _lib.SflError as err:
            assert "no curve" in str(err)
        else:
            raise AssertionError("a batch without a curve answered")
    b.step(c.chunks[1])
    twin.step(c.chunks[1])
    for e, (got, want) in enumerate(zip(sh.snapshot(b, n), sh.snapshot(twin, n))):
        assert not sh.same_env(got, want), f"env {e}: {sh.same_env(got, want)}"
    b.close()
    twin.close()


def _refused(fn, *words):
    try:
        fn()
    except _lib.SflError as err:
        assert all(w in str(err) for w in words), str(err)
    else:
        raise AssertionError(f"not refused (expected {words})")


def run_refusals(lib):
    import ctypes as C
    c = LIFE
    n, cm = n_envs(c), sh.compiled(c.row)
    b = make_batch(c, lib, curve=False)
    _refused(lambda: b.curve_begin(0, 3), "at least 1")
    _refused(lambda: b.curve_begin(4, 3, ring=0), "at least 1")
    _refused(lambda: b.curve_begin(4, 3, series=[5] * n, n_series=5), "series 5 of 5")
    _refused(lambda: b.curve_begin(4, 1 << 20, n_series=1 << 10), "SFL_CURVE_MAX_TABLE_BYTES")
    _refused(lambda: b.curve_begin(4, 3, ring=b.curve_ring_max() + 1), "SFL_CURVE_MAX_RING_BYTES")
    # ring=None: the largest step seen so far (64 if none) + 1; a later step beyond the ring warns once
    assert b.curve_begin(4, 3) == 65
    b.step(20)
    assert b.curve_begin(4, 3) == 21
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        b.step(20)
        assert not seen
        b.step(21)
        b.step(22)
    assert len(seen) == 1 and "more than the curve's ring of 21 rows" in str(seen[0].message)
    b.curve_end()
    b.lib.check(b.lib.dll.sfl_env_begin(b.h), "sfl_env_begin")
    _refused(lambda: b.curve_begin(4, 3), "external-action mode")
    b.close()
    g = make_batch(SERIES[1], lib, curve=False)
    _refused(lambda: g.curve_begin(2, 3, n_series=3), "n_series 3", "group count 2")
    g.close()
    p = make_batch(c, lib, curve=False)
    owner = np.zeros(cm.S, np.int32)
    p.lib.check(p.lib.dll.sfl_part_config(p.h, 0, 1, owner.ctypes.data_as(C.POINTER(C.c_int32)), 0, n, n, 4 * n),
                "sfl_part_config")
    _refused(lambda: p.curve_begin(4, 3), "graph-partitioned")
    p.close()


LIFECYCLE = (run_learn_begin_resets, run_learn_leaves_curve, run_curve_end, run_refusals)
