"""Batch runtime: E lock-step SwitchFL environments + learners on one GPU (one C-ABI handle).

Every env runs the same compiled map with its own seed — the seed the reference
passes both to ``env.reset(seed=...)`` (Flatland's malfunction stream) and to
``np.random.default_rng(seed)`` (the epsilon-greedy stream), distr_q.py:269, 296.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, mfstream
from .compiler import CompiledMap, eps_table, lr_table, NTAB

P = C.POINTER


def _ptr(a: np.ndarray, ctype):
    return a.ctypes.data_as(P(ctype))


def numpy_rng_state(seed: int) -> List[int]:
    """``np.random.default_rng(seed)`` bit-generator state as 5 uint64 words."""
    st = np.random.default_rng(int(seed)).bit_generator.state
    s, inc = int(st["state"]["state"]), int(st["state"]["inc"])
    m = (1 << 64) - 1
    return [s >> 64, s & m, inc >> 64, inc & m, (int(st["has_uint32"]) << 32) | int(st["uinteger"])]


HELD_OUT_EPISODE = _lib.SEED_HELD_OUT_EPISODE
_M64 = (1 << 64) - 1


def _mix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def episode_seed(base: int, k: int) -> int:
    """The seed episode ``k`` of an env created on ``base`` runs on under a seed schedule (include/sfl.h
    sfl_episode_seed): ``base`` itself for k == 0; ``HELD_OUT_EPISODE`` is the index of the held-out exploit rounds.
    Also how an ``EvalBatch`` is given a table's training pool: ``[episode_seed(base, k) for k in range(pool)]``."""
    base, k = int(base) & _M64, int(k) & _M64
    if k == 0:
        return base
    return _mix64((base * 0x9E3779B97F4A7C15 + k * 0xD1B54A32D192ED03 + 0x5EED5C4ED01E5EED) & _M64)


def raw_to_dict(cm: CompiledMap, default_q: float, q: np.ndarray, touched: np.ndarray) -> Dict[tuple, list]:
    """A compact Q block and key-set bitmap (the layout of Batch.q_raw) as the reference's ``q_table`` dict:
    touched rows as {observation tuple: [Q per action]}."""
    bits = np.unpackbits(touched.view(np.uint8), bitorder="little")[:cm.rows_per_env]
    rows = np.nonzero(bits)[0]
    A = cm.arrays
    dq = float(default_q)
    out = {}
    for s in range(cm.S):
        for slot in range(len(cm.ports[s])):
            g = 4 * s + slot
            base, nrows = int(A["row_base"][g]), (1 << len(cm.ports[s])) * cm.K * 3
            sel = rows[(rows >= base) & (rows < base + nrows)]
            if len(sel) == 0:
                continue
            w = int(A["q_w"][g])
            off = int(A["q_off"][g])
            routes = [a for a, (src, _) in enumerate(cm.outcomes[s]) if src == slot] + [int(cm.n_actions[s]) - 1]
            for r in sel:
                stt = int(r) - base
                vals = q[off + stt * w: off + (stt + 1) * w]
                full = [dq] * int(cm.n_actions[s])
                for j, a in enumerate(routes):
                    full[a] = float(vals[j])
                out[cm.obs_of_row(s, slot, stt)] = full
    return out


def row_widths(cm: CompiledMap) -> np.ndarray:
    """Cells of every row id of the map's compact layout ([rows_per_env] uint8; 0 for a row id of no block): block
    g = 4 * switch + in-port slot holds rows row_base[g] + state of q_w[g] cells each."""
    A = cm.arrays
    w = np.zeros(cm.rows_per_env, np.uint8)
    for s in range(cm.S):
        n = (1 << len(cm.ports[s])) * cm.K * 3
        for slot in range(len(cm.ports[s])):
            g = 4 * s + slot
            w[int(A["row_base"][g]): int(A["row_base"][g]) + n] = int(A["q_w"][g])
    return w


def rows_to_dict(cm: CompiledMap, default_q: float, touched: np.ndarray, row_ids: np.ndarray, cells: np.ndarray,
                 widths: Optional[np.ndarray] = None) -> Dict[tuple, list]:
    """``raw_to_dict`` on one env's section of a capture (``Batch.capture``): its key-set words, its live row ids
    (ascending) and their cells as uint64 bit patterns -- the same dict, in the same order, without the dense block.
    A live row whose key bit is clear (values left there by set_q_raw or a shared consensus) is no dict entry, as in
    ``raw_to_dict``.  ``widths``: ``row_widths(cm)``, to share between calls."""
    widths = row_widths(cm) if widths is None else widths
    row_ids = np.asarray(row_ids, np.int64)
    vals = np.ascontiguousarray(cells, np.uint64).view(np.float64)
    start = np.zeros(len(row_ids) + 1, np.int64)
    np.cumsum(widths[row_ids], out=start[1:])
    bits = np.unpackbits(np.ascontiguousarray(touched, np.uint32).view(np.uint8), bitorder="little")
    keyed = bits[row_ids].astype(bool)
    A = cm.arrays
    dq = float(default_q)
    out = {}
    for s in range(cm.S):
        nrows = (1 << len(cm.ports[s])) * cm.K * 3
        for slot in range(len(cm.ports[s])):
            g = 4 * s + slot
            base = int(A["row_base"][g])
            lo, hi = np.searchsorted(row_ids, (base, base + nrows))
            if lo == hi or not keyed[lo:hi].any():
                continue
            routes = [a for a, (src, _) in enumerate(cm.outcomes[s]) if src == slot] + [int(cm.n_actions[s]) - 1]
            na = int(cm.n_actions[s])
            for i in np.nonzero(keyed[lo:hi])[0] + lo:
                v = vals[start[i]: start[i + 1]]
                full = [dq] * na
                for j, a in enumerate(routes):
                    full[a] = float(v[j])
                out[cm.obs_of_row(s, slot, int(row_ids[i]) - base)] = full
    return out


class BatchState:
    """A capture of some envs of a ``Batch`` (``Batch.capture``) as plain numpy arrays, n = the envs captured:
    ``state`` [n][state_bytes] uint8 (one record per env: episode state, RNG, interaction counts, pending-update
    slots, seed), ``touched`` [n][touched_words] uint32 (the key sets), ``row_off`` / ``cell_off`` [n + 1] uint64,
    ``row_ids`` uint32 (each env's live Q rows, ascending) and ``cells`` uint64 (their cells as bit patterns);
    ``seeds`` [n] uint64 (the base seeds); ``sched`` [n][4] float64, the (epsilon, epsilon_decay_rate, lr,
    lr_decay_rate) each env learns with; ``seed_schedule`` the (pool, flags) of the batch's seed schedule ((1, 0), and
    absent from a saved file, for a batch that never left the default); ``fingerprint`` (of the map, gamma, default_q, ntab, max_steps, delay_threshold, the malfunction
    stream's kind and the layout class) and ``layout`` ("lane" or "wave": which kernels' record format)."""

    ARRAYS = (("state", np.uint8), ("touched", np.uint32), ("row_off", np.uint64), ("row_ids", np.uint32),
              ("cell_off", np.uint64), ("cells", np.uint64), ("seeds", np.uint64), ("sched", np.float64))

    def __init__(self, fingerprint: int, layout: str, seed_schedule=(1, 0), **arrays):
        self.fingerprint = int(fingerprint)
        self.layout = str(layout)
        self.seed_schedule = (int(seed_schedule[0]), int(seed_schedule[1]))
        for name, dt in self.ARRAYS:
            setattr(self, name, np.ascontiguousarray(arrays[name], dt))

    def __len__(self):
        return len(self.seeds)

    def save(self, path) -> None:
        """One uncompressed .npz written to exactly ``path``."""
        extra = {} if self.seed_schedule == (1, 0) else {"seed_schedule": np.array(self.seed_schedule, np.uint32)}
        with open(path, "wb") as f:
            np.savez(f, fingerprint=np.array([self.fingerprint], np.uint64),
                     layout=np.array([_lib.STATE_LAYOUTS.index(self.layout)], np.uint32),
                     **{name: getattr(self, name) for name, _ in self.ARRAYS}, **extra)

    @classmethod
    def load(cls, path) -> "BatchState":
        with np.load(path, allow_pickle=False) as z:
            sched = tuple(int(v) for v in z["seed_schedule"]) if "seed_schedule" in z.files else (1, 0)
            return cls(int(z["fingerprint"][0]), _lib.STATE_LAYOUTS[int(z["layout"][0])], seed_schedule=sched,
                       **{name: z[name] for name, _ in cls.ARRAYS})


def dict_to_raw(cm: CompiledMap, default_q: float, table: Dict[tuple, list]) -> Tuple[np.ndarray, np.ndarray]:
    """Inverse of ``raw_to_dict`` (``DistrQLearning.load``): the reference's ``q_table`` dict as a compact Q block and
    key-set bitmap; rejects rows the compact layout cannot hold."""
    A = cm.arrays
    dq = float(default_q)
    q = np.full(cm.q_per_env, dq)
    touched = np.zeros((cm.rows_per_env + 31) // 32, np.uint32)
    sidx = {sid: i for i, sid in enumerate(cm.switch_ids)}
    kidx = {st: i for i, st in enumerate(cm.stations)}
    for key, vals in table.items():
        s = sidx[(int(key[0]), int(key[1]))]
        P_ = len(cm.ports[s])
        sem = key[2:2 + P_]
        tgt = key[2 + P_:2 + 3 * P_]
        dl = key[2 + 3 * P_:2 + 4 * P_]
        slots = [i for i in range(P_) if dl[i] != -1]
        if len(slots) != 1:
            raise ValueError(f"row {key} has no unique in-port")
        slot = slots[0]
        k = kidx[(int(tgt[2 * slot]), int(tgt[2 * slot + 1]))]
        bits = sum(int(b) << j for j, b in enumerate(sem))
        stt = (bits * cm.K + k) * 3 + int(dl[slot])
        g = 4 * s + slot
        w, off = int(A["q_w"][g]), int(A["q_off"][g])
        routes = [a for a, (src, _) in enumerate(cm.outcomes[s]) if src == slot] + [int(cm.n_actions[s]) - 1]
        for a, v in enumerate(vals):
            if a not in routes and float(v) != dq:
                raise ValueError(f"row {key}: action {a} does not leave from the in-port; not representable")
        for j, a in enumerate(routes):
            q[off + stt * w + j] = float(vals[a])
        rid = int(A["row_base"][g]) + stt
        touched[rid >> 5] |= np.uint32(1 << (rid & 31))
    return q, touched


def _descriptors(cm: CompiledMap, hp: dict, max_steps: int, ntab: int, delay_threshold: int):
    """The sfl_map_desc and sfl_hparams of a handle on ``cm`` (Batch and EvalBatch): (map descriptor, hyperparameters,
    the arrays they point at -- to be kept alive until the create call has copied them)."""
    A = cm.arrays
    sc = cm.scenario
    keep = []

    def arr(name, dtype):
        a = np.ascontiguousarray(A[name], dtype=dtype)
        keep.append(a)
        return a

    md = _lib.MapDesc()
    md.H, md.W, md.S, md.T, md.K = cm.H, cm.W, cm.S, cm.T, cm.K
    md.max_episode_steps = sc.max_episode_steps
    md.mf_rate, md.mf_min, md.mf_max = sc.malfunction_rate, sc.malfunction_min, sc.malfunction_max
    md.q_per_env, md.rows_per_env = cm.q_per_env, cm.rows_per_env
    md.delay_threshold = int(delay_threshold)
    spec = [("grid", np.uint16, C.c_uint16), ("cell_sw", np.int16, C.c_int16), ("sw_np", np.uint8, C.c_uint8),
            ("sw_na", np.uint8, C.c_uint8), ("act_src", np.uint8, C.c_uint8), ("act_dst", np.uint8, C.c_uint8),
            ("act_turn", np.uint8, C.c_uint8), ("act_j", np.uint8, C.c_uint8),
            ("first_other", np.uint8, C.c_uint8), ("port_side", np.uint8, C.c_uint8),
            ("slot_nroutes", np.uint8, C.c_uint8), ("slot_route_act", np.uint8, C.c_uint8),
            ("q_w", np.uint8, C.c_uint8), ("port_nb", np.int16, C.c_int16), ("port_len", np.int16, C.c_int16),
            ("port_unique", np.int16, C.c_int16), ("q_off", np.uint64, C.c_uint64),
            ("row_base", np.uint32, C.c_uint32), ("dist", np.int32, C.c_int32),
            ("tr_ed", np.int32, C.c_int32), ("tr_la", np.int32, C.c_int32), ("tr_k", np.int32, C.c_int32),
            ("tr_target", np.int32, C.c_int32), ("tr_init_cell", np.int32, C.c_int32),
            ("tr_init_dist", np.int32, C.c_int32), ("tr_init_delay", np.int32, C.c_int32),
            ("tr_init_dir", np.uint8, C.c_uint8), ("tr_init_port", np.int16, C.c_int16)]
    for name, dt, ct in spec:
        setattr(md, name, _ptr(arr(name, dt), ct))
    eps_tab = eps_table(hp["epsilon"], hp["epsilon_decay_rate"], ntab)
    lr_tab = lr_table(hp["lr"], hp["lr_decay_rate"], ntab)
    h = _lib.HParams()
    h.gamma, h.epsilon, h.epsilon_decay_rate = hp["gamma"], hp["epsilon"], hp["epsilon_decay_rate"]
    h.lr, h.lr_decay_rate, h.default_q = hp["lr"], hp["lr_decay_rate"], hp["default_q"]
    h.max_steps, h.ntab = int(max_steps), int(ntab)
    h.eps_tab, h.lr_tab = _ptr(eps_tab, C.c_double), _ptr(lr_tab, C.c_double)
    keep += [eps_tab, lr_tab]
    return md, h, keep


def _kernel_note(obj) -> str:
    """The handle's kernel note (why it runs the lane-per-env body, "" on a wave kernel): warns, or with
    SFL_REQUIRE_WAVE=1 closes ``obj`` and raises."""
    note = C.create_string_buffer(256)
    obj.lib.check(obj.lib.dll.sfl_get_kernel_note(obj.h, note, 256), "sfl_get_kernel_note")
    text = note.value.decode()
    if text:
        # the lane-per-env body is 15-45x slower than k_wave: say so, or refuse when asked to
        import os
        import warnings
        msg = f"this map runs the lane-per-env kernel (k_run), not k_wave: {text}"
        if os.environ.get("SFL_REQUIRE_WAVE") == "1":
            obj.close()
            raise _lib.SflError(msg)
        warnings.warn(msg, RuntimeWarning, stacklevel=3)
    return text


class Batch:
    """Owns one device handle.  ``hp`` uses the reference's DistrQLearning argument names."""

    def __init__(self, cm: CompiledMap, hp: dict, seeds: Sequence[int], lib: Optional[_lib.Lib] = None,
                 device: int = 0, max_steps: int = 100_000, ntab: int = NTAB, malfunction_stream: str = "counter",
                 delay_threshold: int = 20, hparam_groups: Optional[Sequence[dict]] = None,
                 env_group: Optional[Sequence[int]] = None, seed_pool: int = 1, heldout_exploit: bool = False):
        """``seed_pool`` / ``heldout_exploit``: the seed schedule (``set_seed_schedule``); the defaults replay one
        malfunction realisation per env, as the reference does.
        ``hparam_groups`` / ``env_group``: hyperparameter groups (``set_hparam_groups``) -- env e learns with the
        ``epsilon``, ``epsilon_decay_rate``, ``lr`` and ``lr_decay_rate`` of ``hparam_groups[env_group[e]]``; ``hp``
        still gives ``gamma`` and ``default_q`` (and the schedule of an ungrouped batch).
        ``malfunction_stream``: "counter" (the counter-based draw of the frozen Flatland spec,
        oracle/flatland_lite.py) or "flatland" (ParamMalfunctionGen's np_random draw order, mfstream.py).
        ``delay_threshold``: StandardObserver's (observer.py:221)."""
        self.cm = cm
        self.malfunction_stream = mfstream.check_stream(malfunction_stream)
        self.hp = dict(hp)
        self.seeds = [int(s) for s in seeds]
        self.E = len(self.seeds)
        self.lib = lib or _lib.load_product()
        sc = cm.scenario
        md, h, keep = _descriptors(cm, hp, max_steps, ntab, delay_threshold)  # (alive until sfl_create has copied them)
        self.eps_tab, self.lr_tab = keep[-2], keep[-1]
        seeds_a = np.array(self.seeds, dtype=np.uint64)
        handle = C.c_void_p()
        self.lib.check(self.lib.dll.sfl_create(C.byref(md), C.byref(h), self.E, _ptr(seeds_a, C.c_uint64), device,
                                               C.byref(handle)), "sfl_create")
        self.h = handle
        del md, h, keep
        self.kernel_note = _kernel_note(self)
        if self.malfunction_stream == "flatland":
            tab = mfstream.schedule(self.lib, sc, self.seeds)
            self.lib.check(self.lib.dll.sfl_set_mf_schedule(self.h, tab.shape[1], _ptr(tab, C.c_uint8)),
                           "sfl_set_mf_schedule")
        self.hparam_groups: List[dict] = []
        self.env_group: List[int] = []
        if hparam_groups is not None or env_group is not None:
            try:
                self.set_hparam_groups(hparam_groups, env_group)
            except Exception:
                self.close()
                raise
        if int(seed_pool) != 1 or heldout_exploit:
            try:
                self.set_seed_schedule(seed_pool, heldout_exploit)
            except Exception:
                self.close()
                raise
        self.learn_calls = 0
        self.timed_kernel_ms = 0.0  # device time of the learn / test launches (the phase-timed ones)
        self.trace_env = None
        self.trace_cap = 1 << 16
        self.last_trace = None

    # ------------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.dll.sfl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    GROUP_KEYS = ("epsilon", "epsilon_decay_rate", "lr", "lr_decay_rate")

    def set_hparam_groups(self, hparam_groups: Optional[Sequence[dict]], env_group: Optional[Sequence[int]] = None):
        """Per-env hyperparameter groups (sfl_set_hparam_groups): env e learns with the epsilon and lr schedules of
        ``hparam_groups[env_group[e]]`` (each a dict with ``GROUP_KEYS``; other keys are ignored -- gamma and
        default_q stay the batch's) from the next launch on.  An empty / None ``hparam_groups`` returns every env to
        the batch's own ``hp``."""
        groups = [dict(g) for g in (hparam_groups or [])]
        if not groups:
            if env_group is not None and len(env_group):
                raise ValueError("set_hparam_groups: env_group without hparam_groups")
            self.lib.check(self.lib.dll.sfl_set_hparam_groups(self.h, 0, None, None), "sfl_set_hparam_groups")
            self.hparam_groups, self.env_group = [], []
            return
        if env_group is None or len(env_group) != self.E:
            raise ValueError(f"set_hparam_groups: env_group must name a group for each of the {self.E} envs")
        eg = [int(g) for g in env_group]
        if min(eg) < 0 or max(eg) > 0xFFFF:
            raise ValueError("set_hparam_groups: env_group entries must be in [0, 65535]")
        for g in groups:
            missing = [k for k in self.GROUP_KEYS if k not in g]
            if missing:
                raise ValueError(f"set_hparam_groups: a group lacks {missing}")
        ntab = len(self.eps_tab)
        arr = (_lib.HParamGroup * len(groups))()
        keep = []
        for a, g in zip(arr, groups):
            a.epsilon, a.epsilon_decay_rate = float(g["epsilon"]), float(g["epsilon_decay_rate"])
            a.lr, a.lr_decay_rate = float(g["lr"]), float(g["lr_decay_rate"])
            et = eps_table(g["epsilon"], g["epsilon_decay_rate"], ntab)
            lt = lr_table(g["lr"], g["lr_decay_rate"], ntab)
            keep += [et, lt]
            a.eps_tab, a.lr_tab = _ptr(et, C.c_double), _ptr(lt, C.c_double)
        ega = np.array(eg, dtype=np.uint16)
        self.lib.check(self.lib.dll.sfl_set_hparam_groups(self.h, len(groups), arr, _ptr(ega, C.c_uint16)),
                       "sfl_set_hparam_groups")
        self.hparam_groups, self.env_group = groups, eg

    # ---- seed schedules (sfl_set_seed_schedule): a fresh malfunction stream per episode ----
    def set_seed_schedule(self, pool: int, heldout_exploit: bool = False) -> None:
        """From each env's next reset on, learning episode t of env e (its index since ``learn_begin``; in
        external-action mode the episodes started since begin, minus one) runs on ``episode_seed(seeds[e], t % pool)``
        -- ``pool`` 0: on ``episode_seed(seeds[e], t)``, every episode new -- and a greedy episode (an exploit round,
        ``test``) on ``seeds[e]``, or with ``heldout_exploit`` on ``episode_seed(seeds[e], HELD_OUT_EPISODE)``, which no
        learning episode uses.  ``pool`` 1 without ``heldout_exploit`` is the default.  ``self.seeds`` stay the base
        seeds.  The library refuses (``SflError``) what include/sfl.h lists."""
        pool = int(pool)
        if pool < 0 or pool > 0xFFFFFFFF:
            raise ValueError(f"set_seed_schedule: pool {pool} is not a 32-bit count")
        flags = _lib.SEED_HELDOUT_EXPLOIT if heldout_exploit else 0
        self.lib.check(self.lib.dll.sfl_set_seed_schedule(self.h, pool, flags), "sfl_set_seed_schedule")

    def seed_schedule(self) -> Tuple[int, bool]:
        """(pool, heldout_exploit) as the handle holds them."""
        pool, flags = C.c_uint32(0), C.c_uint32(0)
        self.lib.check(self.lib.dll.sfl_get_seed_schedule(self.h, C.byref(pool), C.byref(flags)), "sfl_get_seed_schedule")
        return int(pool.value), bool(flags.value & _lib.SEED_HELDOUT_EXPLOIT)

    def _seed_schedule_raw(self) -> Tuple[int, int]:
        pool, held = self.seed_schedule()
        return pool, (_lib.SEED_HELDOUT_EXPLOIT if held else 0)

    def episode_seeds(self) -> np.ndarray:
        """[E] uint64: the seed of the episode each env started last (its base seed before its first reset)."""
        out = np.zeros(self.E, np.uint64)
        self.lib.check(self.lib.dll.sfl_get_episode_seeds(self.h, _ptr(out, C.c_uint64)), "sfl_get_episode_seeds")
        return out

    def _qinit_arrays(self):
        cm = self.cm
        keys = sorted(cm.qinit_rows)
        n = len(keys)
        port = np.array([4 * s + slot for s, slot, _ in keys], np.uint32)
        state = np.array([st for _, _, st in keys], np.uint32)
        vals = np.full((n, 4), np.nan)
        for i, k in enumerate(keys):
            row = cm.qinit_rows[k]
            vals[i, :len(row)] = row
        return n, port, state, vals

    def learn_begin(self):
        st = np.array([numpy_rng_state(s) for s in self.seeds], dtype=np.uint64)
        self.lib.check(self.lib.dll.sfl_learn_begin(self.h, _ptr(st, C.c_uint64)), "sfl_learn_begin")

    def apply_qinit(self):
        n, port, state, vals = self._qinit_arrays()
        self.lib.check(self.lib.dll.sfl_apply_qinit(self.h, n, _ptr(port, C.c_uint32), _ptr(state, C.c_uint32),
                                                    _ptr(vals, C.c_double)), "sfl_apply_qinit")

    def _run(self, fn, n_episodes, exploit_freq=0):
        """Run episodes; when ``self.trace_env`` is set, ``self.last_trace`` gets that env's decision trace."""
        E, T = self.E, self.cm.T
        cap = max(1, n_episodes)
        out = dict(cum_reward=np.zeros((cap, E)), arrived=np.zeros((cap, E), np.int32),
                   num_malfunctions=np.zeros((cap, E), np.int32), decisions=np.zeros((cap, E), np.int32),
                   ticks=np.zeros((cap, E), np.int32), delays=np.zeros((cap, T, E), np.int32),
                   cum_reward_exploit=np.zeros((cap, E)), arrived_trains_exploit=np.zeros((cap, E), np.int32))
        a = _lib.RunArgs()
        a.n_episodes, a.exploit_freq, a.stats_cap = n_episodes, exploit_freq, cap
        a.cum_reward = _ptr(out["cum_reward"], C.c_double)
        a.arrived = _ptr(out["arrived"], C.c_int32)
        a.malfunctions = _ptr(out["num_malfunctions"], C.c_int32)
        a.decisions = _ptr(out["decisions"], C.c_int32)
        a.ticks = _ptr(out["ticks"], C.c_int32)
        a.delays = _ptr(out["delays"], C.c_int32)
        a.exploit_cum = _ptr(out["cum_reward_exploit"], C.c_double)
        a.exploit_arrived = _ptr(out["arrived_trains_exploit"], C.c_int32)
        tr = tn = None
        if getattr(self, "trace_env", None) is not None:
            tr = np.zeros((self.trace_cap, 4), np.uint64)
            tn = np.zeros(1, np.uint64)
            a.trace, a.trace_n = _ptr(tr, C.c_uint64), _ptr(tn, C.c_uint64)
            a.trace_env, a.trace_cap = int(self.trace_env), int(self.trace_cap)
        self.lib.check(fn(self.h, C.byref(a)), fn.__name__)
        cnt = self.counters()
        if tr is None and cnt["kernel_variant"] > 0:
            # only the phase-timed instantiation stamps phase cycles: a traced launch (the TRACE kernel) or the
            # lane-per-env body adds kernel time without cycles, which would inflate phase_seconds
            self.timed_kernel_ms += cnt["last_kernel_ms"]
        if tr is not None:
            self.last_trace = tr[:min(int(tn[0]), self.trace_cap)]
        for k in list(out):
            out[k] = out[k][:n_episodes]
        return out

    def learn(self, n_episodes: int, exploit_freq: Optional[int] = None) -> Dict[str, np.ndarray]:
        """``DistrQLearning.learn`` for every env (distr_q.py:244-379); arrays are [episode][env]."""
        f = int(exploit_freq or 0)
        self.learn_begin()
        pre = None
        if f == 1 and n_episodes > 0:
            # the t=0 exploit round runs before __init_q_table (distr_q.py:278-300)
            pre = self.test(1)
            self.lib.check(self.lib.dll.sfl_mark_exploit_done(self.h), "sfl_mark_exploit_done")
        self.apply_qinit()
        out = self._run(self.lib.dll.sfl_learn, n_episodes, f)
        if pre is not None:
            out["cum_reward_exploit"][0] = pre["cum_reward"][0]
            out["arrived_trains_exploit"][0] = pre["arrived"][0]
        self.learn_calls += 1
        return out

    def test(self, n_episodes: int = 1) -> Dict[str, np.ndarray]:
        """``DistrQLearning.test`` greedy episodes (distr_q.py:184-241)."""
        return self._run(self.lib.dll.sfl_test, n_episodes)

    def step(self, decisions_per_env: int) -> Tuple[int, float]:
        """Advance every env by ``decisions_per_env`` learning decisions; returns (total decisions, kernel ms)."""
        n = C.c_uint64(0)
        ms = C.c_double(0.0)
        d = int(decisions_per_env)
        self._largest_step = max(getattr(self, "_largest_step", 0), d)
        ring = getattr(self, "_curve_ring", None)
        if ring is not None and d + 1 > ring and not self._curve_warned:
            import warnings
            self._curve_warned = True
            warnings.warn(f"step({d}) may end up to {d + 1} episodes per env, more than the curve's ring of {ring} rows: "
                          f"the overwritten ones are counted in `lost` (curve_begin(ring={d + 1}) keeps them all)",
                          RuntimeWarning, stacklevel=2)
        f = getattr(self, "_curve_xfreq", None)
        if ring is not None and f and not self._curve_xwarned:
            import math
            import warnings
            p = ring // math.gcd(ring, f)
            if p < d + 1:
                self._curve_xwarned = True
                warnings.warn(f"step({d}) may end up to {d + 1} exploit rounds per env, but rounds {p} apart share a row "
                              f"of the curve's ring ({ring} rows, exploit_freq {f}): the overwritten ones are counted in "
                              f"`exploit_lost` (a ring of {d + 1} or more rows that is coprime to {f} keeps them all)",
                              RuntimeWarning, stacklevel=2)
        self.lib.check(self.lib.dll.sfl_step(self.h, d, C.byref(n), C.byref(ms)), "sfl_step")
        return int(n.value), float(ms.value)

    # ---- step-mode learning curves (sfl_curve_*): the episodes step() ends, reduced on the device ----
    def curve_ring_max(self, exploit: bool = False) -> int:
        """The most ring rows sfl_curve_begin accepts for this batch (SFL_CURVE_MAX_RING_BYTES); ``exploit``: for a
        curve with an exploit record (sfl_curve_exploit: 12 more bytes per row and env)."""
        return max(1, _lib.CURVE_MAX_RING_BYTES // (self.E * (24 + 4 * self.cm.T + (12 if exploit else 0))))

    def curve_begin(self, bin_episodes: int, n_bins: int, series: Optional[Sequence[int]] = None,
                    n_series: Optional[int] = None, ring: Optional[int] = None,
                    exploit_freq: Optional[int] = None) -> int:
        """Start recording learning curves in step mode (include/sfl.h sfl_curve_begin): from now on every ``step``
        folds the episodes it ended into a table of ``n_bins`` x ``n_series`` cells -- episode i of an env in bin
        min(i // bin_episodes, n_bins - 1), env e in series ``series[e]``.  ``series=None``: each env's hyperparameter
        group on a batch that has groups (``n_series`` defaults to the group count), else series 0.  ``n_series``
        defaults to the highest id + 1.  ``ring``: statistics rows kept per env between folds; a ``step(D)`` ends at
        most D + 1 episodes per env, so ``ring >= D + 1`` loses none.  ``ring=None`` picks min(D + 1, the most rows
        ``curve_ring_max()`` allows) with D the largest ``step`` this batch has run so far, or 64 if it has run none;
        a later ``step(D)`` with D + 1 > ring warns once.  Returns the ring size.  Replaces a running curve.

        ``exploit_freq=f`` (f >= 1) also starts the curve's exploit record (``curve_exploit``): ``step`` then runs the
        reference's greedy round before every learning episode t with (t + 1) % f == 0 (distr_q.py:278-281) and
        ``curve()`` reports the rounds as ``exploit_*``.  Rounds ring / gcd(ring, f) apart share a ring row, so
        ``ring=None`` then picks the smallest ring at or above the value described above that is coprime to f (the
        largest one that fits if ``curve_ring_max(exploit=True)`` is below that), and with ``ring >= D + 1`` a
        ``step(D)`` loses no round; with an explicit ring ``step(D)`` warns once if ring / gcd(ring, f) < D + 1."""
        if series is None:
            ptr = None
            n = len(self.hparam_groups) or 1
        else:
            if len(series) != self.E:
                raise ValueError(f"curve_begin: series must name a series for each of the {self.E} envs")
            ids = [int(s) for s in series]
            if min(ids) < 0 or max(ids) > 0xFFFFFFFF:
                raise ValueError("curve_begin: series ids must be non-negative")
            arr = np.array(ids, dtype=np.uint32)
            ptr = _ptr(arr, C.c_uint32)
            n = max(ids) + 1
        n = n if n_series is None else int(n_series)
        f = int(exploit_freq or 0)
        if ring is None:
            import math
            most = self.curve_ring_max(exploit=f > 0)
            ring = min((getattr(self, "_largest_step", 0) or 64) + 1, most)
            if f > 0:
                up = next(r for r in range(ring, ring + f + 1) if math.gcd(r, f) == 1)  # (k f + 1 is coprime to f)
                ring = up if up <= most else next(r for r in range(most, 0, -1) if math.gcd(r, f) == 1)
        self.lib.check(self.lib.dll.sfl_curve_begin(self.h, int(bin_episodes), int(n_bins), n, ptr, int(ring)),
                       "sfl_curve_begin")
        self._curve_shape = (int(n_bins), n)
        self._curve_ring = int(ring)
        self._curve_warned = self._curve_xwarned = False
        self._curve_xfreq = None
        if f > 0:
            self.curve_exploit(f)
        return int(ring)

    def curve_exploit(self, exploit_freq: int) -> None:
        """Start, change or stop the exploit record of the running curve (include/sfl.h sfl_curve_exploit).  f >= 1:
        every later ``step`` runs a greedy round before each learning episode t with (t + 1) % f == 0, as
        ``learn(N, exploit_freq=f)`` does, and folds the rounds it ends into ``curve()``'s ``exploit_*`` cells; the
        call empties those cells and counts rounds from where each env stands.  f == 0: no new round starts, a round in
        flight is finished and folded, the cells stay readable.  Not the reference's: with f == 1 an env standing at
        episode 0 runs its first round on the initialised Q-table (``learn`` runs it before the Q-init rows are
        applied); and greedy decisions count towards ``step``'s decisions per env and ``counters()["decisions"]``,
        as they do in ``learn``."""
        if getattr(self, "_curve_shape", None) is None:
            raise _lib.SflError("curve_exploit: no curve on this batch (curve_begin)")
        f = int(exploit_freq)
        self.lib.check(self.lib.dll.sfl_curve_exploit(self.h, f), "sfl_curve_exploit")
        if f > 0 or self._curve_xfreq is not None:
            self._curve_xfreq = f
            self._curve_xwarned = False

    def curve(self) -> Dict[str, np.ndarray]:
        """The curve so far: one int64 array [n_bins][n_series] per field of sfl_curve_cell (``_lib.CURVE_FIELDS``);
        ``episodes`` [E], each env's learning episodes accounted for (folded or lost); and the float means
        ``arrived_mean``, ``reward_mean``, ``decisions_per_episode``, ``ticks_per_decision``, ``truncated_frac`` and
        ``all_arrived_frac`` over the folded episodes of each cell, NaN where ``count == 0``.  While the curve has an
        exploit record (``curve_begin(exploit_freq=)`` / ``curve_exploit``) also ``exploit_<field>`` for the fields of
        sfl_curve_xcell (``_lib.CURVE_XFIELDS``), ``exploit_rounds`` [E], each env's greedy rounds accounted for, and
        ``exploit_arrived_mean``, ``exploit_reward_mean``, ``exploit_all_arrived_frac`` over the folded rounds of each
        cell, NaN where ``exploit_count == 0``."""
        if getattr(self, "_curve_shape", None) is None:
            raise _lib.SflError("curve: no curve on this batch (curve_begin)")
        nb, ns = self._curve_shape
        cells = np.zeros((nb, ns, len(_lib.CURVE_FIELDS)), np.int64)
        self.lib.check(self.lib.dll.sfl_curve_read(self.h, _ptr(cells, C.c_int64)), "sfl_curve_read")
        ep = np.zeros(self.E, np.int32)
        self.lib.check(self.lib.dll.sfl_curve_episodes(self.h, _ptr(ep, C.c_int32)), "sfl_curve_episodes")
        out = {k: np.ascontiguousarray(cells[:, :, i]) for i, k in enumerate(_lib.CURVE_FIELDS)}
        out["episodes"] = ep
        cnt = out["count"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            per_ep = lambda k: np.where(cnt > 0, out[k] / cnt, np.nan)  # noqa: E731
            out["arrived_mean"] = per_ep("arrived_sum")
            out["reward_mean"] = per_ep("reward_sum")
            out["decisions_per_episode"] = per_ep("decisions_sum")
            out["truncated_frac"] = per_ep("truncated")
            out["all_arrived_frac"] = per_ep("all_arrived")
            out["ticks_per_decision"] = np.where((cnt > 0) & (out["decisions_sum"] > 0),
                                                 out["ticks_sum"] / out["decisions_sum"].astype(np.float64), np.nan)
        if getattr(self, "_curve_xfreq", None) is not None:
            xc = np.zeros((nb, ns, len(_lib.CURVE_XFIELDS)), np.int64)
            self.lib.check(self.lib.dll.sfl_curve_read_exploit(self.h, _ptr(xc, C.c_int64)), "sfl_curve_read_exploit")
            rounds = np.zeros(self.E, np.int32)
            self.lib.check(self.lib.dll.sfl_curve_rounds(self.h, _ptr(rounds, C.c_int32)), "sfl_curve_rounds")
            for i, k in enumerate(_lib.CURVE_XFIELDS):
                out["exploit_" + k] = np.ascontiguousarray(xc[:, :, i])
            out["exploit_rounds"] = rounds
            xn = out["exploit_count"].astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                for k, num in (("arrived_mean", "arrived_sum"), ("reward_mean", "reward_sum"),
                               ("all_arrived_frac", "all_arrived")):
                    out["exploit_" + k] = np.where(xn > 0, out["exploit_" + num] / xn, np.nan)
        return out

    def curve_exploit_fold_ms(self) -> Tuple[float, float]:
        """Device ms of the exploit record's last fold and of all its folds (part of ``curve_fold_ms``'s figures)."""
        last, total = C.c_double(0.0), C.c_double(0.0)
        self.lib.check(self.lib.dll.sfl_curve_exploit_fold_ms(self.h, C.byref(last), C.byref(total)),
                       "sfl_curve_exploit_fold_ms")
        return float(last.value), float(total.value)

    def curve_fold_ms(self) -> Tuple[float, float]:
        """Device ms of the last fold and of all folds since ``curve_begin`` (never part of ``step``'s kernel ms); with
        an exploit record both of its folds."""
        last, total = C.c_double(0.0), C.c_double(0.0)
        self.lib.check(self.lib.dll.sfl_curve_fold_ms(self.h, C.byref(last), C.byref(total)), "sfl_curve_fold_ms")
        return float(last.value), float(total.value)

    def curve_end(self) -> None:
        """Stop recording and free the ring and the table: ``step`` runs as on a batch that never had a curve."""
        self.lib.check(self.lib.dll.sfl_curve_end(self.h), "sfl_curve_end")
        self._curve_shape = self._curve_ring = self._curve_xfreq = None

    PHASES = ("tick", "observe", "egreedy", "apply", "post", "reset", "other")

    def phase_seconds(self) -> Dict[str, float]:
        """Device seconds per phase of the learn loop over this batch's learn / test launches so far: the
        launches' kernel time split by the sampled in-kernel phase cycles (sfl_get_phase_cycles; all zero on the
        lane-per-env body, which has no timers)."""
        cyc = np.zeros(8, np.uint64)
        self.lib.check(self.lib.dll.sfl_get_phase_cycles(self.h, _ptr(cyc, C.c_uint64), 8), "sfl_get_phase_cycles")
        total = float(cyc[7])
        sec = self.timed_kernel_ms * 1e-3
        return {k: (sec * float(cyc[i]) / total if total > 0 else 0.0) for i, k in enumerate(self.PHASES)}

    def counters(self) -> dict:
        c = _lib.Counters()
        self.lib.check(self.lib.dll.sfl_get_counters(self.h, C.byref(c)), "sfl_get_counters")
        return dict(decisions=c.decisions, last_launch_decisions=c.last_launch_decisions,
                    last_launch_ticks=c.last_launch_ticks, last_launch_alg_bytes=c.last_launch_alg_bytes,
                    last_kernel_ms=c.last_kernel_ms, kernel_variant=c.kernel_variant, group_lanes=c.group_lanes)

    # ---- Q-table export / import (the reference's pickle dict, distr_q.py:521-527) -------------
    def q_raw(self, env: int) -> Tuple[np.ndarray, np.ndarray]:
        q = np.zeros(self.cm.q_per_env)
        tw = (self.cm.rows_per_env + 31) // 32
        t = np.zeros(tw, np.uint32)
        self.lib.check(self.lib.dll.sfl_get_q(self.h, env, _ptr(q, C.c_double), _ptr(t, C.c_uint32)), "sfl_get_q")
        return q, t

    def set_q_raw(self, env: int, q: np.ndarray, touched: np.ndarray) -> None:
        """Overwrite one env's compact Q block and key-set bitmap (the layout of q_raw)."""
        q = np.ascontiguousarray(q, np.float64)
        touched = np.ascontiguousarray(touched, np.uint32)
        if q.size != self.cm.q_per_env or touched.size != (self.cm.rows_per_env + 31) // 32:
            raise ValueError("set_q_raw: arrays do not match the map's Q layout")
        self.lib.check(self.lib.dll.sfl_set_q(self.h, env, _ptr(q, C.c_double), _ptr(touched, C.c_uint32)),
                       "sfl_set_q")

    def q_dict(self, env: int) -> Dict[tuple, list]:
        """Touched rows as {observation tuple: [Q per action]} — the reference's ``q_table``."""
        return raw_to_dict(self.cm, self.hp["default_q"], *self.q_raw(env))

    # ---- suspend and resume (sfl_state_*): per-env state and live Q rows, packed on the device ----
    def state_info(self) -> dict:
        d = _lib.StateDesc()
        self.lib.check(self.lib.dll.sfl_state_info(self.h, C.byref(d)), "sfl_state_info")
        return dict(fingerprint=int(d.fingerprint), q_per_env=int(d.q_per_env), state_bytes=int(d.state_bytes),
                    layout=_lib.STATE_LAYOUTS[d.layout], touched_words=int(d.touched_words),
                    rows_per_env=int(d.rows_per_env), seed_offset=int(d.seed_offset))

    def state_ms(self) -> Tuple[float, float]:
        """Device ms of the last capture (its count and gather kernels) and of the last restore."""
        cap, res = C.c_double(0.0), C.c_double(0.0)
        self.lib.check(self.lib.dll.sfl_state_ms(self.h, C.byref(cap), C.byref(res)), "sfl_state_ms")
        return float(cap.value), float(res.value)

    def _sched(self, e: int) -> List[float]:
        """The four schedule values env e learns with: its group's, else the batch's own."""
        src = self.hparam_groups[self.env_group[e]] if self.hparam_groups else self.hp
        return [float(src[k]) for k in self.GROUP_KEYS]

    def _env_list(self, envs, what):
        ids = list(range(self.E)) if envs is None else [int(e) for e in envs]
        if ids and (min(ids) < 0 or max(ids) > 0xFFFFFFFF):
            raise ValueError(f"{what}: env indices must be non-negative")
        return np.array(ids, dtype=np.uint32)

    def _capture(self, envs, with_state: bool):
        """(info, env list, state or None, touched, row_off, row_ids, cell_off, cells) of one device capture."""
        info = self.state_info()
        ids = self._env_list(envs, "capture")
        n = len(ids)
        row_off, cell_off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        self.lib.check(self.lib.dll.sfl_state_capture(self.h, n, _ptr(ids, C.c_uint32), _ptr(row_off, C.c_uint64),
                                                      _ptr(cell_off, C.c_uint64)), "sfl_state_capture")
        state = np.zeros((n, info["state_bytes"]), np.uint8) if with_state else None
        touched = np.zeros((n, info["touched_words"]), np.uint32)
        row_ids, cells = np.zeros(int(row_off[n]), np.uint32), np.zeros(int(cell_off[n]), np.uint64)
        self.lib.check(self.lib.dll.sfl_state_read(self.h, _ptr(state, C.c_uint8) if with_state else None,
                                                   _ptr(touched, C.c_uint32), _ptr(row_ids, C.c_uint32),
                                                   _ptr(cells, C.c_uint64)), "sfl_state_read")
        return info, ids, state, touched, row_off, row_ids, cell_off, cells

    def capture(self, envs: Optional[Sequence[int]] = None) -> BatchState:
        """Everything a launch leaves behind of ``envs`` (default: every env, in order): each env's state record, its
        key set and the live rows of its Q block -- the rows whose key bit is set or that hold a cell other than
        ``default_q`` as a bit pattern -- found and packed on the device (include/sfl.h sfl_state_capture).
        ``restore`` continues them, in this batch or another, bit for bit as if they had never stopped.
        NOT part of the state: ``counters()["decisions"]`` (a handle's own total) and a running curve's cells (start
        a new curve after ``restore``).  The schedule tables are the batch's: the record carries each env's four
        schedule values and ``restore`` checks them."""
        info, ids, state, touched, row_off, row_ids, cell_off, cells = self._capture(envs, True)
        so = info["seed_offset"]
        seeds = np.ascontiguousarray(state[:, so: so + 8]).view(np.uint64).reshape(-1)
        sched = np.array([self._sched(int(e)) for e in ids], np.float64).reshape(len(ids), 4)
        return BatchState(info["fingerprint"], info["layout"], seed_schedule=self._seed_schedule_raw(), state=state, touched=touched, row_off=row_off,
                          row_ids=row_ids, cell_off=cell_off, cells=cells, seeds=seeds, sched=sched)

    def restore(self, state: BatchState, into: Optional[Sequence[int]] = None) -> None:
        """Write the records of ``state`` into the slots ``into`` (default: 0 .. len(state) - 1) of this batch: each
        slot's Q block becomes ``default_q`` plus the record's rows; its key set, env state, RNG stream, interaction
        counts and seed the record's; ``self.seeds`` follows, and with ``malfunction_stream="flatland"`` the schedule is
        expanded again for the new seeds and uploaded.  No other env changes.  Raises ``ValueError`` when a slot's
        four schedule values (its group's, or ``hp``'s) differ bitwise from the ones the env was captured with -- the
        record's interaction counts index those tables, so continuing on other schedules is not a resume --, or when
        the batch's seed schedule is not the one the records were captured under, and
        ``SflError`` for what the library refuses (another map, gamma, default_q, ntab, max_steps, delay_threshold,
        malfunction stream or layout class; a slot out of range or listed twice; inconsistent arrays), leaving the
        batch unchanged.  A running curve does not carry over: call ``curve_begin`` after ``restore``."""
        n = len(state)
        slots = self._env_list(range(n) if into is None else into, "restore")
        if len(slots) != n:
            raise ValueError(f"restore: {len(slots)} slots for {n} records")
        if n and tuple(state.seed_schedule) != self._seed_schedule_raw():
            raise ValueError(f"restore: the batch's seed schedule (pool, flags) = {self._seed_schedule_raw()}, the "
                             f"records were captured under {tuple(state.seed_schedule)}: the running episodes' seeds "
                             "follow from the schedule, so continuing on another one is not a resume")
        for k, e in enumerate(slots):
            if int(e) < self.E:
                mine = np.array(self._sched(int(e)), np.float64)
                if not np.array_equal(mine.view(np.uint64), state.sched[k].view(np.uint64)):
                    raise ValueError(f"restore: slot {int(e)} learns with (epsilon, epsilon_decay_rate, lr, lr_decay_rate) "
                                     f"= {mine.tolist()}, record {k} was captured with {state.sched[k].tolist()}")
        layout = _lib.STATE_LAYOUTS.index(state.layout)
        self.lib.check(self.lib.dll.sfl_state_restore(
            self.h, state.fingerprint, layout, n, _ptr(slots, C.c_uint32), _ptr(state.state, C.c_uint8),
            _ptr(state.touched, C.c_uint32), _ptr(state.row_off, C.c_uint64), _ptr(state.row_ids, C.c_uint32),
            len(state.row_ids), _ptr(state.cell_off, C.c_uint64), _ptr(state.cells, C.c_uint64), len(state.cells)),
            "sfl_state_restore")
        for k, e in enumerate(slots):
            self.seeds[int(e)] = int(state.seeds[k])
        if self.malfunction_stream == "flatland" and n:
            tab = mfstream.schedule(self.lib, self.cm.scenario, self.seeds)
            self.lib.check(self.lib.dll.sfl_set_mf_schedule(self.h, tab.shape[1], _ptr(tab, C.c_uint8)),
                           "sfl_set_mf_schedule")

    def q_dicts(self, envs: Optional[Sequence[int]] = None) -> List[Dict[tuple, list]]:
        """``[q_dict(e) for e in envs]`` (default: every env) from one device capture: only the live rows leave the
        device, not a dense block per env."""
        _, ids, _, touched, row_off, row_ids, cell_off, cells = self._capture(envs, False)
        w = row_widths(self.cm)
        dq = self.hp["default_q"]
        return [rows_to_dict(self.cm, dq, touched[k], row_ids[int(row_off[k]): int(row_off[k + 1])],
                             cells[int(cell_off[k]): int(cell_off[k + 1])], w) for k in range(len(ids))]

    # ---- consensus Q-tables (sfl_consensus): a cohort's learners merged on the device, and shared ----
    def consensus(self, mode: str = "mean", cohorts: Optional[Sequence[Optional[int]]] = None,
                  share: bool = True, n_cohorts: Optional[int] = None) -> float:
        """Merge the envs' Q-tables per cohort (include/sfl.h sfl_consensus): ``mode`` "mean" (of the learned values)
        or "max" (the optimistic merge of distributed Q-learning); ``cohorts[e]`` is env e's cohort id, ``None`` for
        an env that takes no part (default: every env in cohort 0); ``share`` writes each cohort's table back into
        its members; ``n_cohorts`` (default: the highest id + 1) may name more cohorts than have members (their
        table is ``default_q``, their key set empty).  The handle keeps the consensus tables (``consensus_raw`` /
        ``consensus_dict``).  Returns the kernel ms."""
        if mode not in _lib.CONSENSUS_MODES:
            raise ValueError(f"consensus: mode {mode!r} (one of {sorted(_lib.CONSENSUS_MODES)})")
        ms = C.c_double(0.0)
        if cohorts is None:
            n, ptr = 1, None
        else:
            if len(cohorts) != self.E:
                raise ValueError(f"consensus: cohorts must name a cohort (or None) for each of the {self.E} envs")
            ids = [_lib.NO_COHORT if c is None else int(c) for c in cohorts]
            if min(ids) < 0 or max(ids) > _lib.NO_COHORT:
                raise ValueError("consensus: cohort ids must be non-negative")
            arr = np.array(ids, dtype=np.uint32)
            n = max([c + 1 for c in ids if c != _lib.NO_COHORT], default=1)
            ptr = _ptr(arr, C.c_uint32)
        n = n if n_cohorts is None else int(n_cohorts)
        self.lib.check(self.lib.dll.sfl_consensus(self.h, _lib.CONSENSUS_MODES[mode],
                                                  _lib.CONSENSUS_SHARE if share else 0, n, ptr, C.byref(ms)),
                       "sfl_consensus")
        return float(ms.value)

    def consensus_raw(self, cohort: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """The consensus table and key set of one cohort of the last ``consensus`` call, in the layout of q_raw."""
        q = np.zeros(self.cm.q_per_env)
        t = np.zeros((self.cm.rows_per_env + 31) // 32, np.uint32)
        self.lib.check(self.lib.dll.sfl_get_consensus_q(self.h, int(cohort), _ptr(q, C.c_double), _ptr(t, C.c_uint32)),
                       "sfl_get_consensus_q")
        return q, t

    def consensus_dict(self, cohort: int = 0) -> Dict[tuple, list]:
        """One cohort's consensus table as the reference's ``q_table`` dict (the format of q_dict)."""
        return raw_to_dict(self.cm, self.hp["default_q"], *self.consensus_raw(cohort))

    def step_shared(self, decisions_per_env: int, sync_every: int, mode: str = "mean",
                    cohorts: Optional[Sequence[Optional[int]]] = None) -> Tuple[int, float, float]:
        """``decisions_per_env`` learning decisions per env in rounds of ``step(sync_every)`` (the last one shorter),
        each followed by ``consensus(mode, cohorts, share=True)``.  Returns (total decisions, step kernel ms,
        consensus kernel ms)."""
        if decisions_per_env <= 0 or sync_every <= 0:
            raise ValueError("step_shared: decisions_per_env and sync_every must be positive")
        total, step_ms, cons_ms, left = 0, 0.0, 0.0, int(decisions_per_env)
        while left > 0:
            n, ms = self.step(min(int(sync_every), left))
            left -= min(int(sync_every), left)
            total += n
            step_ms += ms
            cons_ms += self.consensus(mode, cohorts, share=True)
        return total, step_ms, cons_ms

    def load_q_dict(self, env: int, table: Dict[tuple, list]):
        """Inverse of ``q_dict`` (``DistrQLearning.load``); rejects rows the compact layout cannot hold."""
        q, touched = dict_to_raw(self.cm, self.hp["default_q"], table)
        self.lib.check(self.lib.dll.sfl_set_q(self.h, env, _ptr(q, C.c_double), _ptr(touched, C.c_uint32)),
                       "sfl_set_q")


class EvalBatch:
    """A read-only bank of ``n_policies`` Q-tables and E envs that each run one greedy episode (``DistrQLearning.test``,
    distr_q.py:184-241) on the table they follow, on their own seed: one evaluation handle (include/sfl.h
    sfl_create_eval).  No env has a table of its own, so scoring a table on thousands of malfunction seeds costs the
    env state only.  The bank is never written: the key-set rows the reference's ``test()`` adds while it looks rows up
    are not recorded (the greedy choices, and every output, are the same)."""

    def __init__(self, cm: CompiledMap, hp: dict, seeds: Sequence[int], n_policies: int,
                 lib: Optional[_lib.Lib] = None, device: int = 0, max_steps: int = 100_000,
                 malfunction_stream: str = "counter", delay_threshold: int = 20):
        self.cm = cm
        self.malfunction_stream = mfstream.check_stream(malfunction_stream)
        self.hp = dict(hp)
        self.seeds = [int(s) for s in seeds]
        self.E = len(self.seeds)
        self.P = int(n_policies)
        self.max_steps = int(max_steps)
        self._rec_envs: List[int] = []
        self._rec_counts: Optional[Tuple[np.ndarray, np.ndarray]] = None  # (of the last evaluate, fetched once)
        self._policy: Optional[np.ndarray] = None
        self.lib = lib or _lib.load_product()
        if self.P < 0 or self.P > 0xFFFFFFFF:
            raise ValueError("EvalBatch: n_policies out of range")
        md, h, keep = _descriptors(cm, hp, max_steps, 1, delay_threshold)  # (a greedy run reads no schedule table)
        seeds_a = np.array(self.seeds, dtype=np.uint64)
        handle = C.c_void_p()
        self.lib.check(self.lib.dll.sfl_create_eval(C.byref(md), C.byref(h), self.E, _ptr(seeds_a, C.c_uint64), device,
                                                    self.P, C.byref(handle)), "sfl_create_eval")
        self.h = handle
        del md, h, keep
        self.kernel_note = _kernel_note(self)
        if self.malfunction_stream == "flatland":
            tab = mfstream.schedule(self.lib, cm.scenario, self.seeds)
            self.lib.check(self.lib.dll.sfl_set_mf_schedule(self.h, tab.shape[1], _ptr(tab, C.c_uint8)),
                           "sfl_set_mf_schedule")

    def close(self):
        if getattr(self, "h", None):
            self.lib.dll.sfl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    counters = Batch.counters

    # ---- the bank's tables ----
    def set_policy_raw(self, p: int, q: np.ndarray, touched: np.ndarray) -> None:
        """Fill table ``p`` from a compact Q block and key-set bitmap (the layout of ``Batch.q_raw``)."""
        q = np.ascontiguousarray(q, np.float64)
        touched = np.ascontiguousarray(touched, np.uint32)
        if q.size != self.cm.q_per_env or touched.size != (self.cm.rows_per_env + 31) // 32:
            raise ValueError("set_policy_raw: arrays do not match the map's Q layout")
        self.lib.check(self.lib.dll.sfl_bank_set(self.h, int(p), _ptr(q, C.c_double), _ptr(touched, C.c_uint32)),
                       "sfl_bank_set")

    def policy_raw(self, p: int) -> Tuple[np.ndarray, np.ndarray]:
        q = np.zeros(self.cm.q_per_env)
        t = np.zeros((self.cm.rows_per_env + 31) // 32, np.uint32)
        self.lib.check(self.lib.dll.sfl_bank_get(self.h, int(p), _ptr(q, C.c_double), _ptr(t, C.c_uint32)), "sfl_bank_get")
        return q, t

    def load_policy_dict(self, p: int, table: Dict[tuple, list]) -> None:
        """Table ``p`` from the reference's ``q_table`` dict (``DistrQLearning.load``), as ``Batch.load_q_dict``."""
        self.set_policy_raw(p, *dict_to_raw(self.cm, self.hp["default_q"], table))

    def policy_dict(self, p: int) -> Dict[tuple, list]:
        return raw_to_dict(self.cm, self.hp["default_q"], *self.policy_raw(p))

    def copy_policy(self, p: int, batch: Batch, env: Optional[int] = None, cohort: Optional[int] = None) -> None:
        """Table ``p`` from a training ``Batch`` on the same device, device to device: env ``env``'s table, or the
        consensus table of cohort ``cohort`` of its last ``consensus`` call (exactly one of the two)."""
        if (env is None) == (cohort is None):
            raise ValueError("copy_policy: give exactly one of env and cohort")
        kind, index = (_lib.BANK_FROM_ENV, env) if cohort is None else (_lib.BANK_FROM_COHORT, cohort)
        if int(index) < 0:
            raise ValueError("copy_policy: a negative index")
        self.lib.check(self.lib.dll.sfl_bank_copy(self.h, int(p), batch.h, kind, int(index)), "sfl_bank_copy")

    # ---- one greedy episode per env ----
    def evaluate(self, env_policy: Optional[Sequence[int]] = None, per_env: bool = True) -> Dict[str, object]:
        """Every env runs one greedy episode from a reset on table ``env_policy[e]`` (default ``e % n_policies``).
        Returns ``policy`` [E]; with ``per_env`` the arrays ``cum_reward``, ``arrived``, ``num_malfunctions``,
        ``decisions``, ``ticks``, ``truncated`` [E] and ``delays``, ``at_dest`` [T][E]; and ``table``: the int64 fields
        of sfl_eval_cell (``_lib.EVAL_FIELDS``) as [P] arrays, reduced on the device, plus the means ``early_mean``,
        ``late_mean``, ``not_arrived_mean`` (trains per episode), ``reward_mean``, ``decisions_per_episode``,
        ``ticks_per_decision``, ``truncated_frac`` and ``all_arrived_frac`` -- NaN where a policy has no episode."""
        E, T = self.E, self.cm.T
        if env_policy is None:
            pol = (np.arange(E, dtype=np.int64) % max(self.P, 1)).astype(np.uint32)
        else:
            if len(env_policy) != E:
                raise ValueError(f"evaluate: env_policy must name a policy for each of the {E} envs")
            ids = np.asarray(env_policy, dtype=np.int64)
            if ids.min() < 0 or ids.max() > 0xFFFFFFFF:
                raise ValueError("evaluate: policy ids must be non-negative")
            pol = ids.astype(np.uint32)
        out: Dict[str, object] = {}
        o = _lib.EvalOut()
        if per_env:
            out = dict(cum_reward=np.zeros(E), arrived=np.zeros(E, np.int32), num_malfunctions=np.zeros(E, np.int32),
                       decisions=np.zeros(E, np.int32), ticks=np.zeros(E, np.int32), truncated=np.zeros(E, np.int32),
                       delays=np.zeros((T, E), np.int32), at_dest=np.zeros((T, E), np.uint8))
            o.cum_reward = _ptr(out["cum_reward"], C.c_double)
            o.arrived = _ptr(out["arrived"], C.c_int32)
            o.malfunctions = _ptr(out["num_malfunctions"], C.c_int32)
            o.decisions = _ptr(out["decisions"], C.c_int32)
            o.ticks = _ptr(out["ticks"], C.c_int32)
            o.truncated = _ptr(out["truncated"], C.c_int32)
            o.delays = _ptr(out["delays"], C.c_int32)
            o.at_dest = _ptr(out["at_dest"], C.c_uint8)
        self.lib.check(self.lib.dll.sfl_bank_eval(self.h, _ptr(pol, C.c_uint32), C.byref(o)), "sfl_bank_eval")
        cells = np.zeros((self.P, len(_lib.EVAL_FIELDS)), np.int64)
        self.lib.check(self.lib.dll.sfl_bank_read(self.h, _ptr(cells, C.c_int64)), "sfl_bank_read")
        out["policy"] = pol
        out["table"] = eval_table(cells)
        self._policy = pol
        self._rec_counts = None
        return out

    def fold_ms(self) -> Tuple[float, float]:
        """Device ms of the last fold and of all folds of this handle (never part of ``counters()['last_kernel_ms']``)."""
        last, total = C.c_double(0.0), C.c_double(0.0)
        self.lib.check(self.lib.dll.sfl_bank_fold_ms(self.h, C.byref(last), C.byref(total)), "sfl_bank_fold_ms")
        return float(last.value), float(total.value)


    # ---- why trains did not arrive ----
    def diagnose(self, stall: int = 30, per_env: bool = True) -> Dict[str, object]:
        """Classify every train of every episode of the last ``evaluate`` on the device (include/sfl.h sfl_bank_diag
        states the rule; ``CLASS_NAMES`` names the values): a train is stalled when it stood on its final cell over the
        last ``stall`` ticks.  May be called again with another ``stall`` without evaluating again.  Returns, with
        ``per_env``, ``cls`` (uint8), ``blocker`` (int16, -1: none) and ``stalled_for`` (int32, -1: off the map) as
        [T][E]; and ``table``: the int64 fields of sfl_diag_cell (``_lib.DIAG_FIELDS``) as [P] arrays, reduced on the
        device, plus per-episode means ``<class>_mean`` of the six class counts and ``jammed_frac`` -- NaN where a
        policy has no episode."""
        E, T = self.E, self.cm.T
        out: Dict[str, object] = {}
        o = _lib.DiagOut()
        if per_env:
            out = dict(cls=np.zeros((T, E), np.uint8), blocker=np.zeros((T, E), np.int16),
                       stalled_for=np.zeros((T, E), np.int32))
            o.cls = _ptr(out["cls"], C.c_uint8)
            o.blocker = _ptr(out["blocker"], C.c_int16)
            o.stalled_for = _ptr(out["stalled_for"], C.c_int32)
        stall = int(stall)
        if not -2**31 <= stall < 2**31:
            raise ValueError("diagnose: stall out of range")
        self.lib.check(self.lib.dll.sfl_bank_diag(self.h, stall, C.byref(o)), "sfl_bank_diag")
        cells = np.zeros((self.P, len(_lib.DIAG_FIELDS)), np.int64)
        self.lib.check(self.lib.dll.sfl_bank_diag_read(self.h, _ptr(cells, C.c_int64)), "sfl_bank_diag_read")
        out["stall"] = stall
        out["table"] = diag_table(cells)
        return out

    def hotspots(self, p: int) -> np.ndarray:
        """[H][W] uint32: per cell of the map, the stalled trains (classes stop_loop, deadlock_queue, deadlock_cycle) of
        policy ``p``'s episodes that stand on it, from the last ``diagnose``."""
        if int(p) < 0 or int(p) > 0xFFFFFFFF:
            raise ValueError("hotspots: policy id out of range")
        hot = np.zeros((self.cm.H, self.cm.W), np.uint32)
        self.lib.check(self.lib.dll.sfl_bank_diag_hot(self.h, int(p), _ptr(hot, C.c_uint32)), "sfl_bank_diag_hot")
        return hot

    def diag_ms(self) -> Tuple[float, float]:
        """Device ms of the last diagnosis (classify and fold) and of all of this handle (never part of
        ``counters()['last_kernel_ms']``)."""
        last, total = C.c_double(0.0), C.c_double(0.0)
        self.lib.check(self.lib.dll.sfl_bank_diag_ms(self.h, C.byref(last), C.byref(total)), "sfl_bank_diag_ms")
        return float(last.value), float(total.value)


    # ---- episodes recorded on the device ----
    def record(self, envs: Optional[Sequence[int]], max_ticks: Optional[int] = None,
               max_decisions: Optional[int] = None) -> None:
        """Arm a recording of the listed envs (distinct, any order; slot k is ``envs[k]``) for every later ``evaluate``
        (include/sfl.h sfl_bank_record states what is recorded); ``None`` or an empty list disarms it.  ``max_ticks``
        defaults to the map's ``max_episode_steps`` -- a tick at that horizon ends the episode, so no frame is cut --
        and ``max_decisions`` to ``min(max_steps + 1, 4096)``."""
        envs = [] if envs is None else [int(e) for e in envs]
        self._rec_counts = None
        if any(e < 0 or e > 0xFFFFFFFF for e in envs):
            raise ValueError("record: env ids must be non-negative")
        if not envs:
            self.lib.check(self.lib.dll.sfl_bank_record(self.h, 0, None, 0, 0), "sfl_bank_record")
            self._rec_envs = []
            return
        ticks = int(self.cm.scenario.max_episode_steps if max_ticks is None else max_ticks)
        decs = int(min(self.max_steps + 1, 4096) if max_decisions is None else max_decisions)
        if not (-2**31 <= ticks < 2**31 and -2**31 <= decs < 2**31):
            raise ValueError("record: max_ticks / max_decisions out of range")
        a = np.array(envs, dtype=np.uint32)
        self.lib.check(self.lib.dll.sfl_bank_record(self.h, len(envs), _ptr(a, C.c_uint32), ticks, decs), "sfl_bank_record")
        self._rec_envs = envs

    def record_info(self) -> Dict[str, int]:
        """The armed recording: ``n`` (0: none), ``tick_cap``, ``dec_cap``, ``dec_words``."""
        o = _lib.RecordInfo()
        self.lib.check(self.lib.dll.sfl_bank_record_info(self.h, C.byref(o)), "sfl_bank_record_info")
        return dict(n=int(o.n), tick_cap=int(o.tick_cap), dec_cap=int(o.dec_cap), dec_words=int(o.dec_words))

    def recording(self, k: int) -> "Episode":
        """Slot ``k`` of the recording, as the last ``evaluate`` filled it: the episode of env ``record``'s ``envs[k]``."""
        info = self.record_info()
        n, T = info["n"], self.cm.T
        if int(k) < 0 or int(k) > 0xFFFFFFFF:
            raise ValueError("recording: slot out of range")
        if self._rec_counts is None:  # (every slot's counts in one call, kept until the next evaluate / record)
            ticks, decs = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
            self.lib.check(self.lib.dll.sfl_bank_record_counts(self.h, _ptr(ticks, C.c_int32), _ptr(decs, C.c_int32)),
                           "sfl_bank_record_counts")
            self._rec_counts = (ticks, decs)
        ticks, decs = self._rec_counts
        cell = np.zeros((info["tick_cap"], T), np.int32)
        bits = np.zeros((info["tick_cap"], T), np.uint32)
        rows = np.zeros((info["dec_cap"], info["dec_words"]), np.int32)
        self.lib.check(self.lib.dll.sfl_bank_record_read(self.h, int(k), _ptr(cell, C.c_int32), _ptr(bits, C.c_uint32),
                                                         _ptr(rows, C.c_int32)), "sfl_bank_record_read")
        env = self._rec_envs[int(k)]
        return Episode.from_raw(self.cm, env, self.seeds[env], int(self._policy[env]), int(ticks[k]), int(decs[k]),
                                cell, bits, rows)

    def traffic(self, p: int) -> Dict[str, np.ndarray]:
        """The recorded frames and decisions of the slots whose env followed policy ``p`` in the last ``evaluate``,
        reduced on the device (include/sfl.h sfl_bank_record_traffic): ``occupancy``, ``standing``,
        ``standing_malfunction`` as [H][W] and ``decisions``, ``stops`` as [S] uint32 arrays."""
        if int(p) < 0 or int(p) > 0xFFFFFFFF:
            raise ValueError("traffic: policy id out of range")
        H, W, S = self.cm.H, self.cm.W, self.cm.S
        out = {k: np.zeros((H, W) if i < 3 else (S,), np.uint32) for i, k in enumerate(_lib.TRAFFIC_FIELDS)}
        o = _lib.RecordTraffic()
        for k in _lib.TRAFFIC_FIELDS:
            setattr(o, k, _ptr(out[k], C.c_uint32))
        self.lib.check(self.lib.dll.sfl_bank_record_traffic(self.h, int(p), C.byref(o)), "sfl_bank_record_traffic")
        return out

    def record_ms(self) -> Tuple[float, float]:
        """Device ms of the last traffic fold and of all of this handle."""
        last, total = C.c_double(0.0), C.c_double(0.0)
        self.lib.check(self.lib.dll.sfl_bank_record_ms(self.h, C.byref(last), C.byref(total)), "sfl_bank_record_ms")
        return float(last.value), float(total.value)


class Episode:
    """One recorded bank episode (``EvalBatch.recording``): ``env``, ``seed``, ``policy``; the episode's true ``ticks``
    and ``n_decisions`` and ``complete`` (both within the recording's caps); the kept frames ``cell`` (int32, -1 off
    the map), ``heading``, ``state`` (index into ``_lib.TRAIN_STATES``) and ``malfunction`` (the counter) as
    [frames][T], frame i after tick i + 1; and ``decisions``: one [rows] int array per field of
    ``_lib.REC_DEC_FIELDS`` plus ``obs`` ([rows] observation tuples, ``CompiledMap.obs_of_row``) and ``agent`` (the
    deciding switches' names)."""

    def __init__(self, env, seed, policy, ticks, n_decisions, tick_cap, dec_cap, cell, heading, state, malfunction,
                 decisions):
        self.env, self.seed, self.policy = int(env), int(seed), int(policy)
        self.ticks, self.n_decisions = int(ticks), int(n_decisions)
        self.tick_cap, self.dec_cap = int(tick_cap), int(dec_cap)
        self.cell, self.heading, self.state, self.malfunction = cell, heading, state, malfunction
        self.decisions = decisions

    @property
    def complete(self) -> bool:
        return self.ticks <= self.tick_cap and self.n_decisions <= self.dec_cap

    @property
    def frames(self) -> int:
        return int(self.cell.shape[0])

    @property
    def rows(self) -> int:
        return int(self.decisions["now"].shape[0])

    @classmethod
    def from_raw(cls, cm: CompiledMap, env, seed, policy, ticks, n_decisions, cell, bits, rows) -> "Episode":
        """From a slot's arrays as sfl_bank_record_read returns them ([tick_cap][T], [tick_cap][T], [dec_cap][words]):
        cut to the kept frames and rows, the state word taken apart, the observations decoded."""
        nf, nr = min(ticks, cell.shape[0]), min(n_decisions, rows.shape[0])
        b = bits[:nf]
        dec = {k: np.ascontiguousarray(rows[:nr, i]) for i, k in enumerate(_lib.REC_DEC_FIELDS)}
        dec["obs"] = [cm.obs_of_row(int(s), int(sl), int(st)) for s, sl, st in zip(dec["switch"], dec["slot"], dec["state"])]
        dec["agent"] = ["switch_%d-%d" % tuple(cm.switch_ids[int(s)]) for s in dec["switch"]]
        return cls(env, seed, policy, ticks, n_decisions, cell.shape[0], rows.shape[0], np.ascontiguousarray(cell[:nf]),
                   (b & 3).astype(np.uint8), ((b >> 2) & 7).astype(np.uint8), ((b >> 13) & 0xFF).astype(np.uint8), dec)

    def save(self, path) -> None:
        """One ``.npz``: the scalars, the frame arrays, the decision fields, the observation tuples (padded to the
        longest, with their lengths) and the agents' names."""
        meta = np.array([self.env, self.seed, self.policy, self.ticks, self.n_decisions, self.tick_cap, self.dec_cap],
                        np.int64)
        obs = self.decisions["obs"]
        olen = np.array([len(o) for o in obs], np.int32)
        opad = -np.ones((len(obs), int(olen.max()) if len(obs) else 0), np.int32)
        for i, o in enumerate(obs):
            opad[i, :len(o)] = o
        np.savez_compressed(path, meta=meta, cell=self.cell, heading=self.heading, state=self.state,
                            malfunction=self.malfunction, obs=opad, obs_len=olen,
                            agent=np.array(self.decisions["agent"], dtype=np.str_),
                            **{"dec_" + k: self.decisions[k] for k in _lib.REC_DEC_FIELDS})

    @classmethod
    def load(cls, path) -> "Episode":
        with np.load(path) as z:
            dec = {k: z["dec_" + k] for k in _lib.REC_DEC_FIELDS}
            dec["obs"] = [tuple(int(x) for x in row[:n]) for row, n in zip(z["obs"], z["obs_len"])]
            dec["agent"] = [str(x) for x in z["agent"]]
            return cls(*[int(x) for x in z["meta"]], z["cell"], z["heading"], z["state"], z["malfunction"], dec)


# include/sfl.h SFL_DIAG_*: the class a diagnosis gives a train, by value
CLASS_NAMES = dict(enumerate(_lib.DIAG_CLASSES))


def diag_table(cells: np.ndarray) -> Dict[str, np.ndarray]:
    """sfl_diag_cell words [P][12] as one [P] int64 array per field plus, per episode, the means of the six class counts
    (``truncated_mean`` ... ``deadlock_cycle_mean``) and ``jammed_frac`` (NaN without episodes)."""
    t = {k: np.ascontiguousarray(cells[:, i]) for i, k in enumerate(_lib.DIAG_FIELDS)}
    n = t["episodes"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in _lib.DIAG_CLASSES[1:]:
            t[k + "_mean"] = np.where(n > 0, t[k] / n, np.nan)
        t["jammed_frac"] = np.where(n > 0, t["episodes_jammed"] / n, np.nan)
    return t


def eval_table(cells: np.ndarray) -> Dict[str, np.ndarray]:
    """sfl_eval_cell words [P][15] as one [P] int64 array per field plus the per-episode means (NaN without episodes)."""
    t = {k: np.ascontiguousarray(cells[:, i]) for i, k in enumerate(_lib.EVAL_FIELDS)}
    n = t["episodes"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_ep = lambda k: np.where(n > 0, t[k] / n, np.nan)  # noqa: E731
        t["early_mean"] = per_ep("trains_early")
        t["late_mean"] = per_ep("trains_late")
        t["not_arrived_mean"] = per_ep("trains_not_arrived")
        t["reward_mean"] = per_ep("reward_sum")
        t["decisions_per_episode"] = per_ep("decisions_sum")
        t["truncated_frac"] = per_ep("truncated")
        t["all_arrived_frac"] = per_ep("all_arrived")
        t["ticks_per_decision"] = np.where((n > 0) & (t["decisions_sum"] > 0),
                                           t["ticks_sum"] / t["decisions_sum"].astype(np.float64), np.nan)
    return t
