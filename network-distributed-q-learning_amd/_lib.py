"""ctypes binding of include/sfl.h.

The product loads ``libsfl.so`` (built for gfx950 by build.py) and nothing else:
there is no CPU fallback.  ``load(path)`` also serves the test-only host build
(``libsfl_hostsim.so``), which tests/ use to check the kernel body against the
oracle without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(HERE, "libsfl.so")
ABI_VERSION = 9  # include/sfl.h SFL_ABI_VERSION

P = C.POINTER


class MapDesc(C.Structure):
    _fields_ = [
        ("H", C.c_int32), ("W", C.c_int32), ("S", C.c_int32), ("T", C.c_int32), ("K", C.c_int32),
        ("max_episode_steps", C.c_int32), ("mf_rate", C.c_double), ("mf_min", C.c_int32), ("mf_max", C.c_int32),
        ("q_per_env", C.c_uint64), ("rows_per_env", C.c_uint32),
        ("grid", P(C.c_uint16)), ("cell_sw", P(C.c_int16)),
        ("sw_np", P(C.c_uint8)), ("sw_na", P(C.c_uint8)), ("act_src", P(C.c_uint8)), ("act_dst", P(C.c_uint8)),
        ("act_turn", P(C.c_uint8)), ("act_j", P(C.c_uint8)), ("first_other", P(C.c_uint8)),
        ("port_side", P(C.c_uint8)), ("slot_nroutes", P(C.c_uint8)), ("slot_route_act", P(C.c_uint8)),
        ("q_w", P(C.c_uint8)), ("port_nb", P(C.c_int16)), ("port_len", P(C.c_int16)), ("port_unique", P(C.c_int16)),
        ("q_off", P(C.c_uint64)), ("row_base", P(C.c_uint32)), ("dist", P(C.c_int32)),
        ("tr_ed", P(C.c_int32)), ("tr_la", P(C.c_int32)), ("tr_k", P(C.c_int32)), ("tr_target", P(C.c_int32)),
        ("tr_init_cell", P(C.c_int32)), ("tr_init_dist", P(C.c_int32)), ("tr_init_delay", P(C.c_int32)),
        ("tr_init_dir", P(C.c_uint8)), ("tr_init_port", P(C.c_int16)), ("delay_threshold", C.c_int32),
    ]


class HParams(C.Structure):
    _fields_ = [
        ("gamma", C.c_double), ("epsilon", C.c_double), ("epsilon_decay_rate", C.c_double), ("lr", C.c_double),
        ("lr_decay_rate", C.c_double), ("default_q", C.c_double), ("max_steps", C.c_int64), ("ntab", C.c_int32),
        ("eps_tab", P(C.c_double)), ("lr_tab", P(C.c_double)),
    ]


class HParamGroup(C.Structure):
    """sfl_hparam_group: one group's epsilon / lr schedule (sfl_set_hparam_groups)."""
    _fields_ = [
        ("epsilon", C.c_double), ("epsilon_decay_rate", C.c_double), ("lr", C.c_double), ("lr_decay_rate", C.c_double),
        ("eps_tab", P(C.c_double)), ("lr_tab", P(C.c_double)),
    ]


MAX_HPARAM_GROUPS = 4096  # include/sfl.h SFL_MAX_HPARAM_GROUPS
# include/sfl.h SFL_CONSENSUS_*
CONSENSUS_MODES = {"mean": 0, "max": 1}
CONSENSUS_SHARE = 1
NO_COHORT = 0xFFFFFFFF
CONSENSUS_CHUNK = 256
# include/sfl.h sfl_curve_cell: the 16 int64 words of a cell in order, and SFL_CURVE_MAX_*
CURVE_FIELDS = ("count", "lost", "arrived_sum", "arrived_min", "arrived_max", "all_arrived", "reward_sum", "reward_min",
                "reward_max", "decisions_sum", "ticks_sum", "malfunctions_sum", "delay_sum", "truncated", "first_episode",
                "last_episode")
# include/sfl.h sfl_curve_xcell: the 11 int64 words of an exploit cell in order
CURVE_XFIELDS = ("count", "lost", "arrived_sum", "arrived_min", "arrived_max", "all_arrived", "reward_sum", "reward_min",
                 "reward_max", "first_episode", "last_episode")
# include/sfl.h sfl_eval_cell: the 15 int64 words of a policy's cell in order, and SFL_BANK_FROM_*
EVAL_FIELDS = ("episodes", "trains_early", "trains_late", "trains_not_arrived", "arrived_min", "arrived_max", "all_arrived",
               "reward_sum", "reward_min", "reward_max", "decisions_sum", "ticks_sum", "malfunctions_sum",
               "delay_sum_arrived", "truncated")
# include/sfl.h sfl_diag_cell: the 12 int64 words of a policy's non-arrival cell in order, and SFL_DIAG_* (class values)
DIAG_FIELDS = ("episodes", "truncated", "never_departed", "moving_late", "stop_loop", "deadlock_queue", "deadlock_cycle",
               "cycles", "episodes_jammed", "stalled_in_malfunction", "stalled_for_sum", "stalled_for_max")
DIAG_CLASSES = ("arrived", "truncated", "never_departed", "moving_late", "stop_loop", "deadlock_queue", "deadlock_cycle")
# include/sfl.h SFL_REC_*: the words of a recorded decision's row in order, the size limit of a recording, and the fields
# of sfl_record_traffic
REC_DEC_FIELDS = ("now", "switch", "train", "slot", "state", "mask", "action", "reward", "next_switch", "step_now")
REC_MAX_BYTES = 1 << 30
TRAFFIC_FIELDS = ("occupancy", "standing", "standing_malfunction", "decisions", "stops")
TRAIN_STATES = ("WAITING", "READY_TO_DEPART", "MALFUNCTION_OFF_MAP", "MOVING", "STOPPED", "MALFUNCTION", "DONE")
BANK_FROM_ENV = 0
BANK_FROM_COHORT = 1
CURVE_MAX_TABLE_BYTES = 64 << 20
CURVE_MAX_RING_BYTES = 1 << 30


class RunArgs(C.Structure):
    _fields_ = [
        ("n_episodes", C.c_int32), ("exploit_freq", C.c_int32), ("stats_cap", C.c_int32), ("pad_", C.c_int32),
        ("cum_reward", P(C.c_double)), ("arrived", P(C.c_int32)), ("malfunctions", P(C.c_int32)),
        ("decisions", P(C.c_int32)), ("ticks", P(C.c_int32)), ("delays", P(C.c_int32)),
        ("exploit_cum", P(C.c_double)), ("exploit_arrived", P(C.c_int32)),
        ("trace", P(C.c_uint64)), ("trace_n", P(C.c_uint64)), ("trace_env", C.c_int32), ("trace_cap", C.c_int32),
    ]


class Counters(C.Structure):
    _fields_ = [("decisions", C.c_uint64), ("last_launch_decisions", C.c_uint64),
                ("last_launch_ticks", C.c_uint64), ("last_launch_alg_bytes", C.c_uint64),
                ("last_kernel_ms", C.c_double), ("kernel_variant", C.c_int32), ("group_lanes", C.c_int32)]


class EnvIO(C.Structure):
    """sfl_env_io (external-action mode)."""
    _fields_ = [("actions", P(C.c_int32)), ("agent", P(C.c_int32)), ("train", P(C.c_int32)), ("slot", P(C.c_int32)),
                ("state", P(C.c_uint32)), ("mask", P(C.c_uint32)), ("reward", P(C.c_int32)), ("now", P(C.c_int32)),
                ("next_switch", P(C.c_int32)), ("step_now", P(C.c_int32)), ("arrived", P(C.c_uint32)),
                ("malfunctions", P(C.c_int32)), ("delays", P(C.c_int32)), ("truncated", P(C.c_int32))]


class EvalOut(C.Structure):
    """sfl_eval_out: the optional per-env outputs of sfl_bank_eval."""
    _fields_ = [("cum_reward", P(C.c_double)), ("arrived", P(C.c_int32)), ("malfunctions", P(C.c_int32)),
                ("decisions", P(C.c_int32)), ("ticks", P(C.c_int32)), ("truncated", P(C.c_int32)),
                ("delays", P(C.c_int32)), ("at_dest", P(C.c_uint8))]


class DiagOut(C.Structure):
    """sfl_diag_out: the optional per-train outputs of sfl_bank_diag."""
    _fields_ = [("cls", P(C.c_uint8)), ("blocker", P(C.c_int16)), ("stalled_for", P(C.c_int32))]


class RecordInfo(C.Structure):
    """sfl_record_info: what sfl_bank_record_info reports of the armed recording."""
    _fields_ = [("n", C.c_uint32), ("tick_cap", C.c_int32), ("dec_cap", C.c_int32), ("dec_words", C.c_uint32)]


class RecordTraffic(C.Structure):
    """sfl_record_traffic: the optional outputs of sfl_bank_record_traffic."""
    _fields_ = [("occupancy", P(C.c_uint32)), ("standing", P(C.c_uint32)), ("standing_malfunction", P(C.c_uint32)),
                ("decisions", P(C.c_uint32)), ("stops", P(C.c_uint32))]


class StateDesc(C.Structure):
    """sfl_state_desc: what sfl_state_info reports of a handle's state records."""
    _fields_ = [("fingerprint", C.c_uint64), ("q_per_env", C.c_uint64), ("state_bytes", C.c_uint32),
                ("layout", C.c_uint32), ("touched_words", C.c_uint32), ("rows_per_env", C.c_uint32),
                ("seed_offset", C.c_uint32), ("pad_", C.c_uint32)]


STATE_LAYOUTS = ("lane", "wave")  # include/sfl.h SFL_STATE_LANE, SFL_STATE_WAVE
OBS_WIDTH = 18    # include/sfl.h SFL_OBS_WIDTH
MAX_ACTIONS = 16  # include/sfl.h SFL_MAX_ACTIONS


class EnvDevIO(C.Structure):
    """sfl_env_dev_io (external-action mode, device pointers)."""
    _fields_ = [("io", EnvIO), ("obs", P(C.c_int32)), ("action_mask", P(C.c_uint8)), ("n_actions", P(C.c_int32)),
                ("done", P(C.c_uint8))]


DEST_BONUS = 1000  # include/sfl.h SFL_DEST_BONUS


class EnvTransIO(C.Structure):
    """sfl_env_trans_io (external-action mode's transition ring, device pointers)."""
    _fields_ = [("capacity", C.c_uint32), ("pad_", C.c_uint32), ("env", P(C.c_int32)), ("train", P(C.c_int32)),
                ("now", P(C.c_int32)), ("agent", P(C.c_int32)), ("action", P(C.c_int32)), ("reward", P(C.c_int32)),
                ("next_agent", P(C.c_int32)), ("next_n_actions", P(C.c_int32)), ("terminal", P(C.c_uint8)),
                ("obs", P(C.c_int32)), ("next_obs", P(C.c_int32)), ("next_action_mask", P(C.c_uint8)),
                ("total", P(C.c_int64)), ("last_count", P(C.c_int32)), ("dropped", P(C.c_int64))]


EXPORTS = {
    "sfl_abi_version": (C.c_int, []),
    "sfl_build_id": (C.c_char_p, []),
    "sfl_last_error": (C.c_char_p, []),
    "sfl_device_count": (C.c_int, [P(C.c_int)]),
    "sfl_create": (C.c_int, [P(MapDesc), P(HParams), C.c_uint32, P(C.c_uint64), C.c_int, P(C.c_void_p)]),
    "sfl_destroy": (C.c_int, [C.c_void_p]),
    "sfl_learn_begin": (C.c_int, [C.c_void_p, P(C.c_uint64)]),
    "sfl_apply_qinit": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_uint32), P(C.c_uint32), P(C.c_double)]),
    "sfl_mark_exploit_done": (C.c_int, [C.c_void_p]),
    "sfl_learn": (C.c_int, [C.c_void_p, P(RunArgs)]),
    "sfl_test": (C.c_int, [C.c_void_p, P(RunArgs)]),
    "sfl_step": (C.c_int, [C.c_void_p, C.c_int64, P(C.c_uint64), P(C.c_double)]),
    "sfl_get_q": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_double), P(C.c_uint32)]),
    "sfl_set_q": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_double), P(C.c_uint32)]),
    "sfl_get_counters": (C.c_int, [C.c_void_p, P(Counters)]),
    "sfl_get_kernel_note": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
    # external-action mode (aec.py) and the per-phase device time (distr_q.py timing accumulators)
    "sfl_env_begin": (C.c_int, [C.c_void_p]),
    "sfl_env_begin_wave": (C.c_int, [C.c_void_p]),
    "sfl_env_step": (C.c_int, [C.c_void_p, P(EnvIO)]),
    "sfl_env_step_dev": (C.c_int, [C.c_void_p, P(EnvDevIO)]),
    "sfl_env_sync": (C.c_int, [C.c_void_p]),
    "sfl_env_trans_begin": (C.c_int, [C.c_void_p, P(EnvTransIO)]),
    "sfl_env_trans_end": (C.c_int, [C.c_void_p]),
    "sfl_get_obs_tables": (C.c_int, [C.c_void_p, P(C.c_int32), P(C.c_int32)]),
    "sfl_get_phase_cycles": (C.c_int, [C.c_void_p, P(C.c_uint64), C.c_int32]),
    "sfl_get_env_state": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_int32), P(C.c_int32), P(C.c_uint64),
                                    P(C.c_int32), P(C.c_uint32)]),
    # Flatland-compatible malfunction stream (mfstream.py)
    "sfl_set_mf_schedule": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_uint8)]),
    "sfl_mf_schedule_flatland": (C.c_int, [P(C.c_uint32), C.c_int32, P(C.c_int32), C.c_int32, C.c_int32, C.c_double,
                                           C.c_int32, C.c_int32, C.c_int32, P(C.c_uint8)]),
    # graph-partitioned mode (partition.py)
    "sfl_part_config": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, P(C.c_int32), C.c_uint32, C.c_uint32,
                                  C.c_uint32, C.c_uint32]),
    "sfl_part_record_sizes": (C.c_int, [P(C.c_uint32), P(C.c_uint32)]),
    "sfl_part_begin": (C.c_int, [C.c_void_p]),
    "sfl_part_local": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, P(C.c_uint64)]),
    "sfl_part_owner": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "sfl_part_counts": (C.c_int, [C.c_void_p, P(C.c_uint32), C.c_int32]),
    "sfl_part_set_caps": (C.c_int, [C.c_void_p, C.c_uint32]),
    "sfl_get_sync_count": (C.c_int, [C.c_void_p, P(C.c_uint64), P(C.c_uint64)]),
    "sfl_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sfl_part_set_local_rows": (C.c_int, [C.c_void_p, P(C.c_uint8)]),
    "sfl_part_get_q": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_double), P(C.c_uint32)]),
    # hyperparameter groups (runtime.Batch hparam_groups, sweep.py)
    "sfl_set_hparam_groups": (C.c_int, [C.c_void_p, C.c_int32, P(HParamGroup), P(C.c_uint16)]),
    # seed schedules (runtime.Batch seed_pool / set_seed_schedule / episode_seeds); sfl_episode_seed, the one entry
    # point that returns a uint64_t, is bound beside this table (Lib.__init__)
    "sfl_set_seed_schedule": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "sfl_get_seed_schedule": (C.c_int, [C.c_void_p, P(C.c_uint32), P(C.c_uint32)]),
    "sfl_get_episode_seeds": (C.c_int, [C.c_void_p, P(C.c_uint64)]),
    # consensus Q-tables (runtime.Batch consensus / consensus_raw)
    "sfl_consensus": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, P(C.c_uint32), P(C.c_double)]),
    "sfl_get_consensus_q": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_double), P(C.c_uint32)]),
    # step-mode learning curves (runtime.Batch curve_begin / curve / curve_end)
    "sfl_curve_begin": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, P(C.c_uint32), C.c_int32]),
    "sfl_curve_read": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "sfl_curve_episodes": (C.c_int, [C.c_void_p, P(C.c_int32)]),
    "sfl_curve_fold_ms": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double)]),
    "sfl_curve_end": (C.c_int, [C.c_void_p]),
    # the curve's exploit record (runtime.Batch curve_begin(exploit_freq=) / curve_exploit)
    "sfl_curve_exploit": (C.c_int, [C.c_void_p, C.c_int32]),
    "sfl_curve_read_exploit": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "sfl_curve_rounds": (C.c_int, [C.c_void_p, P(C.c_int32)]),
    "sfl_curve_exploit_fold_ms": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double)]),
    # policy-bank evaluation (runtime.EvalBatch)
    "sfl_create_eval": (C.c_int, [P(MapDesc), P(HParams), C.c_uint32, P(C.c_uint64), C.c_int, C.c_uint32, P(C.c_void_p)]),
    "sfl_bank_set": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_double), P(C.c_uint32)]),
    "sfl_bank_get": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_double), P(C.c_uint32)]),
    "sfl_bank_copy": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_uint32]),
    "sfl_bank_eval": (C.c_int, [C.c_void_p, P(C.c_uint32), P(EvalOut)]),
    "sfl_bank_read": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "sfl_bank_fold_ms": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double)]),
    "sfl_bank_diag": (C.c_int, [C.c_void_p, C.c_int32, P(DiagOut)]),
    "sfl_bank_diag_read": (C.c_int, [C.c_void_p, P(C.c_int64)]),
    "sfl_bank_diag_hot": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_uint32)]),
    "sfl_bank_diag_ms": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double)]),
    "sfl_bank_record": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_uint32), C.c_int32, C.c_int32]),
    "sfl_bank_record_info": (C.c_int, [C.c_void_p, P(RecordInfo)]),
    "sfl_bank_record_counts": (C.c_int, [C.c_void_p, P(C.c_int32), P(C.c_int32)]),
    "sfl_bank_record_read": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_int32), P(C.c_uint32), P(C.c_int32)]),
    "sfl_bank_record_traffic": (C.c_int, [C.c_void_p, C.c_uint32, P(RecordTraffic)]),
    "sfl_bank_record_ms": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double)]),
    # suspend and resume (runtime.Batch capture / restore / q_dicts)
    "sfl_state_info": (C.c_int, [C.c_void_p, P(StateDesc)]),
    "sfl_state_capture": (C.c_int, [C.c_void_p, C.c_uint32, P(C.c_uint32), P(C.c_uint64), P(C.c_uint64)]),
    "sfl_state_read": (C.c_int, [C.c_void_p, P(C.c_uint8), P(C.c_uint32), P(C.c_uint32), P(C.c_uint64)]),
    "sfl_state_restore": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, P(C.c_uint32), P(C.c_uint8),
                                    P(C.c_uint32), P(C.c_uint64), P(C.c_uint32), C.c_uint64, P(C.c_uint64),
                                    P(C.c_uint64), C.c_uint64]),
    "sfl_state_ms": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double)]),
}


SEED_HELD_OUT_EPISODE = 0xFFFFFFFFFFFFFFFF  # SFL_SEED_HELD_OUT_EPISODE
SEED_HELDOUT_EXPLOIT = 1                    # SFL_SEED_HELDOUT_EXPLOIT


class SflError(RuntimeError):
    pass


class Lib:
    def __init__(self, path: str):
        if not os.path.exists(path):
            raise SflError(f"{path} not found — build it first (python -c 'import __graft_entry__ as g; g.build()')")
        self.path = path
        self.dll = C.CDLL(path)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(self.dll, name)
            fn.restype = res
            fn.argtypes = args
        self.dll.sfl_episode_seed.restype = C.c_uint64
        self.dll.sfl_episode_seed.argtypes = [C.c_uint64, C.c_uint64]
        if self.dll.sfl_abi_version() != ABI_VERSION:
            raise SflError("ABI version mismatch")
        self.build_id = self.dll.sfl_build_id().decode()
        self.defines = ""
        self.flags = ""
        self.experimental = False

    def check_fresh(self, allow_experimental: bool = False):
        """Refuse a library that is not the product build of the sources in this tree: a stale build, or a
        tuning / experiment build (its -D defines or flags are part of its build id).  With
        ``allow_experimental`` a build of these sources with the defines it records is accepted
        (``self.defines`` then names them); experiment switches make its results invalid."""
        from . import build
        want = build.product_build_id()
        self.defines = build.built_defines(self.path) or ""
        self.flags = build.built_flags(self.path) or ""
        tuned = bool(self.defines or self.flags)
        if self.build_id == want and not tuned:
            self.experimental = False
            return
        if allow_experimental and tuned and self.build_id == build.build_id(self.defines.split(), self.flags.split()):
            self.experimental = True
            return
        what = f"defines: {self.defines or '-'}, flags: {self.flags or '-'}"
        if tuned and allow_experimental:
            raise SflError(f"{self.path} is stale: a tuning / experiment build ({what}) of other sources than the "
                           f"tree's (rebuild it)")
        if tuned:
            raise SflError(f"{self.path} is a tuning / experiment build ({what}), not the product library; set "
                           f"SFL_EXPERIMENTAL=1 (bench.py --experimental) to run it anyway")
        raise SflError(f"{self.path} is stale: built as {self.build_id[:12]}, the tree's product build is {want[:12]} "
                       f"(rebuild: python -c 'import __graft_entry__ as g; g.build()')")

    def check(self, rc: int, what: str):
        if rc != 0:
            raise SflError(f"{what}: {self.dll.sfl_last_error().decode(errors='replace')}")

    def device_count(self) -> int:
        n = C.c_int(0)
        self.dll.sfl_device_count(C.byref(n))
        return n.value


_product = None


def load_product() -> Lib:
    """The HIP library; raises if it is missing or no GPU is visible (no fallback)."""
    global _product
    if _product is None:
        # one HIP runtime per process: load torch's (it carries its own libamdhip64.so.7 / HSA runtime)
        # before libsfl.so resolves the same soname, so the library and torch's RCCL / allocator share it
        import torch  # noqa: F401

        # SFL_LIB: an alternative in-tree build of the same HIP sources (tuning sweeps); accepted only with
        # SFL_EXPERIMENTAL=1 unless it is the product build itself (check_fresh)
        lib = Lib(os.environ.get("SFL_LIB", PRODUCT_LIB))
        lib.check_fresh(allow_experimental=os.environ.get("SFL_EXPERIMENTAL") == "1")
        if lib.device_count() < 1:
            raise SflError("libsfl.so loaded but no HIP device is visible: the SwitchFL hot path runs on MI355X only")
        _product = lib
    return _product
