"""External-action mode: E SwitchFL environments stepped one decision per call by a policy on the host.

The reference's plugin surface between learner and env is the PettingZoo AEC protocol
(switchfl/switch_env.py:616-675): ``for agent in env.agent_iter(): obs, reward, term, trunc, info =
env.last(); ...; env.step(action)``, driven by any learner (distr_q.py:302-320).  The fused device loop
(runtime.Batch) runs the reference's own learner; this module exposes the env alone through
``sfl_env_begin`` / ``sfl_env_step`` (include/sfl.h): every call applies each env's action to the
observation the previous call emitted and runs the env on to its next decision (or episode end), on the
device, for all E envs at once.  ``ASyncSwitchEnv`` (env.py) wraps env 0 of an ``AECBatch`` in the
reference's single-env methods.  For a policy that lives on the same GPU, ``AECBatch.step_torch`` / ``sync``
(``sfl_env_step_dev`` / ``sfl_env_sync``) are the same step with torch tensors on the device in and out, the
observation vector decoded on the device, and no host wait.  ``kernel="wave"`` (or
``SFL_ENV_KERNEL=wave``) runs the same env step on the handle's wave kernel -- one env per wavefront or lane group,
``sfl_env_begin_wave`` -- instead of the lane-per-env body: same calls, same results.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from .compiler import CompiledMap
from .runtime import Batch, _ptr

# the learner's hyper-parameters do not enter the env (no epsilon draw, no Q-table access)
DEST_BONUS = _lib.DEST_BONUS  # include/sfl.h SFL_DEST_BONUS: the reward of a terminal transition (transitions_begin)
ACTION_RESET = -2  # include/sfl.h SFL_ACTION_RESET: reset the env where it stands (env.reset() mid-episode)
_STREAM_DEFAULT = 1  # include/sfl.h SFL_STREAM_DEFAULT: the device's default stream (its own handle is null)
_ENV_HP = dict(gamma=1.0, epsilon=0.0, epsilon_decay_rate=1.0, lr=0.0, lr_decay_rate=1.0, default_q=0.0)


class AECBatch:
    """E plain environments (no learner) on one device handle, stepped by ``step(actions)``.

    After each call, for env e: ``agent[e]`` is the deciding switch of its pending observation (-1: its
    episode ended in this call; the next call starts the next one), ``train``, ``slot``, ``state``
    (the observation index, ``observation(e)`` gives the reference's int64 vector), ``mask`` (action
    mask bits), ``reward`` (last()'s reward of (switch, train)), ``now``; for the action applied in this
    call ``next_switch`` and ``step_now`` (-1 if none); ``arrived`` (bitmask, 4 words); at an episode end
    ``malfunctions``, ``delays`` [T] and ``truncated``.

    ``kernel``: ``"lane"`` -- the lane-per-env body (``sfl_env_begin``) --, ``"wave"`` -- the wave kernel of the
    handle's shape (``sfl_env_begin_wave``; ``batch.counters()`` reports ``kernel_variant`` and ``group_lanes``) --
    or None: ``os.environ.get("SFL_ENV_KERNEL", "lane")``, read at creation like ``SFL_KERNEL`` and ``SFL_WAVE_G``.
    Both give the same outputs bit for bit.  ``"wave"`` raises ``SflError`` with the library's reason where it cannot
    be honoured (a map without a wave shape, ``SFL_KERNEL=scalar``, the host build); any other value ``ValueError``.

    ``seed_pool``: the seed schedule (``Batch.set_seed_schedule``): the n-th episode an env starts (n = 0, 1, ...; an
    ``ACTION_RESET`` starts one like an episode end does) runs on ``runtime.episode_seed(seeds[e], n % seed_pool)``, with
    0 on ``episode_seed(seeds[e], n)``.  The default, 1, replays one malfunction realisation per env, as the reference.
    ``batch.episode_seeds()`` reads the running episodes' seeds.
    """

    KERNELS = ("lane", "wave")

    FIELDS = ("agent", "train", "slot", "state", "mask", "reward", "now", "next_switch", "step_now", "malfunctions",
              "truncated")

    def __init__(self, cm: CompiledMap, seeds: Sequence[int], lib: Optional[_lib.Lib] = None, device: int = 0,
                 max_steps: int = 100_000, malfunction_stream: str = "counter", delay_threshold: int = 20,
                 kernel: Optional[str] = None, seed_pool: int = 1):
        if kernel is None:
            kernel = os.environ.get("SFL_ENV_KERNEL", "lane")
        if kernel not in self.KERNELS:
            raise ValueError(f"AECBatch: kernel {kernel!r} is none of {self.KERNELS}")
        self.kernel = kernel
        self.cm = cm
        self.batch = Batch(cm, _ENV_HP, seeds, lib=lib, device=device, max_steps=max_steps, ntab=16,
                           malfunction_stream=malfunction_stream, delay_threshold=delay_threshold, seed_pool=seed_pool)
        self.lib = self.batch.lib
        self.E = self.batch.E
        E, T = self.E, cm.T
        self.out = {k: np.zeros(E, np.uint32 if k in ("state", "mask") else np.int32) for k in self.FIELDS}
        self.out["arrived"] = np.zeros((4, E), np.uint32)
        self.out["delays"] = np.zeros((T, E), np.int32)
        self._io = _lib.EnvIO()
        for k, ct in (("agent", C.c_int32), ("train", C.c_int32), ("slot", C.c_int32), ("state", C.c_uint32),
                      ("mask", C.c_uint32), ("reward", C.c_int32), ("now", C.c_int32), ("next_switch", C.c_int32),
                      ("step_now", C.c_int32), ("arrived", C.c_uint32), ("malfunctions", C.c_int32),
                      ("delays", C.c_int32), ("truncated", C.c_int32)):
            setattr(self._io, k, _ptr(self.out[k], ct))
        self._act = np.full(E, -1, np.int32)
        self.device = device
        self._t = None            # step_torch's tensors and descriptor (made by its first call)
        self._stream = None       # the stream last handed to the library (step_torch on a HIP device)
        self._host_stale = False  # device steps ran since the host arrays (self.out) were last filled
        self._trans = None        # the transition ring's tensors and descriptor (transitions_begin)
        try:
            if kernel == "wave":
                self.lib.check(self.lib.dll.sfl_env_begin_wave(self.batch.h), "sfl_env_begin_wave")
            else:
                self.lib.check(self.lib.dll.sfl_env_begin(self.batch.h), "sfl_env_begin")
        except Exception:
            self.batch.close()
            raise

    def close(self):
        self.batch.close()

    # ---- the policy on the device: tensors in and out, no host in the loop -------------------------------
    TORCH_FIELDS = FIELDS + ("arrived", "delays", "obs", "action_mask", "n_actions", "done")

    def _torch_setup(self, torch):
        E, T = self.E, self.cm.T
        # the host build's "device" memory is host memory: the same path on CPU tensors
        on_gpu = self.lib.device_count() > 0
        dev = torch.device("cuda", self.device) if on_gpu else torch.device("cpu")
        i32 = dict(dtype=torch.int32, device=dev)
        out = {k: torch.zeros(E, **i32) for k in self.FIELDS}
        out["arrived"] = torch.zeros((4, E), **i32)
        out["delays"] = torch.zeros((T, E), **i32)
        out["obs"] = torch.zeros((E, _lib.OBS_WIDTH), **i32)
        out["action_mask"] = torch.zeros((E, _lib.MAX_ACTIONS), dtype=torch.uint8, device=dev)
        out["n_actions"] = torch.zeros(E, **i32)
        out["done"] = torch.zeros(E, dtype=torch.uint8, device=dev)
        dio = _lib.EnvDevIO()
        for k, ct in (("agent", C.c_int32), ("train", C.c_int32), ("slot", C.c_int32), ("state", C.c_uint32),
                      ("mask", C.c_uint32), ("reward", C.c_int32), ("now", C.c_int32), ("next_switch", C.c_int32),
                      ("step_now", C.c_int32), ("arrived", C.c_uint32), ("malfunctions", C.c_int32),
                      ("delays", C.c_int32), ("truncated", C.c_int32)):
            setattr(dio.io, k, C.cast(out[k].data_ptr(), _lib.P(ct)))
        dio.obs = C.cast(out["obs"].data_ptr(), _lib.P(C.c_int32))
        dio.action_mask = C.cast(out["action_mask"].data_ptr(), _lib.P(C.c_uint8))
        dio.n_actions = C.cast(out["n_actions"].data_ptr(), _lib.P(C.c_int32))
        dio.done = C.cast(out["done"].data_ptr(), _lib.P(C.c_uint8))
        self._t = dict(out=out, dio=dio, dev=dev, on_gpu=on_gpu, none=torch.full((E,), -1, **i32), act=None)
        return self._t

    def _follow_stream(self, torch, t):
        if t["on_gpu"]:
            # the library follows the stream the tensors are produced on (sfl_set_stream synchronises: only on a change)
            s = torch.cuda.current_stream(t["dev"]).cuda_stream or _STREAM_DEFAULT
            if s != self._stream:
                self.lib.check(self.lib.dll.sfl_set_stream(self.batch.h, C.c_void_p(s)), "sfl_set_stream")
                self._stream = s

    # ---- learner transitions assembled on the device (include/sfl.h sfl_env_trans_*) ----------
    TRANS_FIELDS = ("env", "train", "now", "agent", "action", "reward", "next_agent", "next_n_actions")

    def transitions_begin(self, capacity: Optional[int] = None):
        """Start the transition assembler: from now on every ``step`` / ``step_torch`` call is followed, on the device
        and on the same stream, by the learner's bookkeeping (the reference's ``update_dict``, distr_q.py:322-356), which
        appends complete transitions to a replay ring of ``capacity`` rows (default ``2 * E``).  Returns the ring, a dict
        of tensors on the handle's device (CPU tensors with the host build), which ``transitions()`` returns too:
        ``env``, ``train``, ``now``, ``agent``, ``action``, ``reward``, ``next_agent``, ``next_n_actions`` int32 [N];
        ``terminal`` uint8 [N]; ``obs``, ``next_obs`` int32 [N, 18]; ``next_action_mask`` uint8 [N, 16]; ``total``
        int64 [1] (rows since begin: row g is in slot ``g % N``), ``last_count`` int32 [1] (rows of the last call) and
        ``dropped`` int64 [E] (pending entries discarded at episode ends and resets).  A row is
        ``(agent, obs, action) -> reward, (next_agent, next_obs, next_action_mask)``; a terminal row (the train arrived)
        has ``reward == DEST_BONUS``, ``terminal == 1``, ``next_agent == -1``, ``next_obs`` all -1 and a zero mask;
        after a STOP ``agent == next_agent``.  Order: calls, envs ascending, and within an env the row of the deciding
        train first, then the terminal rows by train and switch.  Nothing waits for the device; the tensors are
        rewritten in place by later calls.  Sampling a minibatch without leaving the device::

            ring = batch.transitions_begin(capacity=1 << 20)
            ...                                        # out = batch.step_torch(policy(out)), many times
            n = ring["total"].clamp(max=ring["env"].numel())          # rows that are valid, a tensor: no .item()
            idx = torch.randint(0, 1 << 31, (256,), device=n.device) % n.clamp(min=1)
            obs, act, rew = ring["obs"][idx], ring["action"][idx], ring["reward"][idx]
            nobs, nmask, term = ring["next_obs"][idx], ring["next_action_mask"][idx], ring["terminal"][idx]
        """
        import torch
        if capacity is None:
            capacity = 2 * self.E
        if not isinstance(capacity, int) or isinstance(capacity, bool) or capacity < 1 or capacity > 0x7FFFFFFF:
            raise ValueError(f"transitions_begin: capacity {capacity!r} (an int of 1 .. 2^31 - 1)")
        t = self._t or self._torch_setup(torch)
        self._follow_stream(torch, t)
        dev, N = t["dev"], capacity
        ring = {k: torch.zeros(N, dtype=torch.int32, device=dev) for k in self.TRANS_FIELDS}
        ring["terminal"] = torch.zeros(N, dtype=torch.uint8, device=dev)
        ring["obs"] = torch.zeros((N, _lib.OBS_WIDTH), dtype=torch.int32, device=dev)
        ring["next_obs"] = torch.zeros((N, _lib.OBS_WIDTH), dtype=torch.int32, device=dev)
        ring["next_action_mask"] = torch.zeros((N, _lib.MAX_ACTIONS), dtype=torch.uint8, device=dev)
        ring["total"] = torch.zeros(1, dtype=torch.int64, device=dev)
        ring["last_count"] = torch.zeros(1, dtype=torch.int32, device=dev)
        ring["dropped"] = torch.zeros(self.E, dtype=torch.int64, device=dev)
        io = _lib.EnvTransIO()
        io.capacity = N
        for k, ct in _lib.EnvTransIO._fields_[2:]:
            setattr(io, k, C.cast(ring[k].data_ptr(), ct))
        self.lib.check(self.lib.dll.sfl_env_trans_begin(self.batch.h, C.byref(io)), "sfl_env_trans_begin")
        self._trans = dict(ring=ring, io=io)
        return ring

    def transitions(self):
        """The ring ``transitions_begin`` returned (None: no assembler is running)."""
        return self._trans["ring"] if self._trans else None

    def transitions_end(self) -> None:
        """Stop the assembler: later calls leave the ring as it is (the tensors stay valid)."""
        self.lib.check(self.lib.dll.sfl_env_trans_end(self.batch.h), "sfl_env_trans_end")
        self._trans = None

    def step_torch(self, actions=None):
        """``step`` for a policy that lives on the handle's device: ``actions`` is an int32 tensor [E] on that device
        (None: no actions), the result a dict of tensors on it -- the ``FIELDS`` of ``step`` (all int32: ``state``,
        ``mask`` and ``arrived`` hold the same bits as the uint32 host arrays), ``arrived`` [4, E], ``delays`` [T, E],
        and the decoded decision: ``obs`` [E, 18] int32 (``observation(e)`` padded to four ports with -1),
        ``action_mask`` [E, 16] uint8 (columns past ``n_actions`` are 0), ``n_actions`` [E] and ``done`` [E] uint8 (the episode ended in this call: the
        row is -1, the mask 0, n_actions 0).  The tensors are allocated once and are views valid until the next
        call.  The call is queued on torch's current stream and returns without waiting for the device.  There is
        no range check on the host (the deciding agents are on the device): an action outside a switch's action
        space is refused by the kernel, the same observation is emitted again, and ``sync()`` raises.  With the
        host build (tests) the tensors are CPU tensors and the same path runs on the caller's thread."""
        import torch
        t = self._t or self._torch_setup(torch)
        if actions is None:
            a = t["none"]
        else:
            if not isinstance(actions, torch.Tensor) or actions.dtype != torch.int32:
                raise ValueError("step_torch: actions must be an int32 tensor")
            if tuple(actions.shape) != (self.E,) or not actions.is_contiguous():
                raise ValueError(f"step_torch: actions of shape {tuple(actions.shape)} for {self.E} envs (contiguous [E])")
            if actions.device != t["dev"]:
                raise ValueError(f"step_torch: actions on {actions.device}, the envs are on {t['dev']}")
            a = actions
        self._follow_stream(torch, t)
        t["act"] = a  # (alive until the next call: the kernel reads it after this call returned)
        t["dio"].io.actions = C.cast(a.data_ptr(), _lib.P(C.c_int32))
        self._host_stale = True
        self.lib.check(self.lib.dll.sfl_env_step_dev(self.batch.h, C.byref(t["dio"])), "sfl_env_step_dev")
        return t["out"]

    def sync(self) -> None:
        """Wait for the device steps queued so far; raises ``SflError`` if an env reported an error (a refused action)."""
        self.lib.check(self.lib.dll.sfl_env_sync(self.batch.h), "sfl_env_sync")

    def step(self, actions: Optional[Sequence[int]] = None) -> Dict[str, np.ndarray]:
        """Apply ``actions[e]`` to each env's pending observation (None / < 0: none; ``ACTION_RESET``: reset the env
        where it stands) and run every env to its next observation or episode end.  Returns the output arrays (views, valid until the next call)."""
        if self._host_stale:
            # device steps (step_torch) ran since the host arrays were filled: a call without actions re-emits every
            # env's pending observation into them (the range check below reads the deciding agents from there)
            self._host_stale = False
            self._io.actions = None
            self.lib.check(self.lib.dll.sfl_env_step(self.batch.h, C.byref(self._io)), "sfl_env_step")
        if actions is None:
            self._act[:] = -1
        else:
            a = np.asarray(actions, np.int64)
            if a.shape != (self.E,):
                raise ValueError(f"step: {a.shape} actions for {self.E} envs")
            # the reference asserts action_space(agent).contains(action) (switch_env.py:213-215)
            ag = self.out["agent"]
            pend = (ag >= 0) & (a >= 0)
            na = np.asarray(self.cm.n_actions, np.int64)[np.where(pend, ag, 0)]
            bad = np.nonzero(pend & (a >= na))[0]
            if len(bad):
                e = int(bad[0])
                raise ValueError(f"step: action {int(a[e])} of env {e} is outside switch {int(ag[e])}'s action space "
                                 f"Discrete({int(na[e])})")
            self._act[:] = np.where(a == ACTION_RESET, ACTION_RESET, np.where(a < 0, -1, a)).astype(np.int32)
        self._io.actions = _ptr(self._act, C.c_int32)
        self.lib.check(self.lib.dll.sfl_env_step(self.batch.h, C.byref(self._io)), "sfl_env_step")
        return self.out

    # ---- the reference's views of one env's pending decision ----------------------------------------
    def observation(self, e: int) -> np.ndarray:
        """observer.py:303-306: [r, c, sem[P], target[2P], delay[P]] (int64)."""
        s = int(self.out["agent"][e])
        if s < 0:
            return None
        return np.array(self.cm.obs_of_row(s, int(self.out["slot"][e]), int(self.out["state"][e])), np.int64)

    def action_mask(self, e: int) -> np.ndarray:
        s = int(self.out["agent"][e])
        n = int(self.cm.n_actions[s])
        m = int(self.out["mask"][e])
        return np.array([(m >> a) & 1 for a in range(n)], np.int8)

    def arrived_trains(self, e: int) -> List[int]:
        w = self.out["arrived"][:, e]
        return [h for h in range(self.cm.T) if (int(w[h >> 5]) >> (h & 31)) & 1]

    def agent_name(self, s: int) -> str:
        r, c = self.cm.switch_ids[s]
        return f"switch_{r}-{c}"

    def semaphores(self, e: int) -> dict:
        """Env e's semaphore table in the reference's format {port node: [owner, 'in'|'out', direction, t0, t1]}
        (rail_network.py:303-416; direction = map_direction(port), port_side)."""
        from .parity import env_state
        sem = env_state(self.batch, e)[2]
        side = self.cm.arrays["port_side"]
        out = {}
        for s, ports in enumerate(self.cm.ports):
            for j, node in enumerate(ports):
                r = int(sem[4 * s + j])
                if not (r >> 41) & 1:
                    continue
                t0 = (r & 0xFFFF) - ((r & 0x8000) << 1)
                t1 = ((r >> 16) & 0xFFFF) - (((r >> 16) & 0x8000) << 1)
                out[node] = [(r >> 32) & 0xFF, "in" if (r >> 40) & 1 else "out", int(side[4 * s + j]), t0, t1]
        return out

