"""No case of tests/test_phase_scalars_gpu.py is vacuous, shown on the host build and the oracle alone; and the
``--counter lgkm`` mode of scripts/load_chains.py counts what it says, while the default mode prints what it printed.

Shares: a condition that is meant to change what every env computes (gamma and default_q, the lr decay, the other
malfunction stream, the delay threshold) must change the result of at least three quarters of the 63 envs against the
base run with the same seeds; a condition that depends on where an env happens to stand (the table's end crossed
inside a launch, a greedy round cut by a one-decision launch) must hold in at least three quarters of the envs looked
at.  The seeds are tests/_sempass.py's, for which the host build meets every share."""
import os
import sys

import numpy as np
import pytest

from tests import _decide_loads as D
from tests import _phase_scalars as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import load_chains as lc  # noqa: E402

CFGS = ("c3", "c2")


def test_variant_7_maps_are_variant_7_shapes():
    cm = D.compiled("c3")
    assert (cm.S, cm.T) == (64, 32)


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("cond", ("gamma", "lr_in", "flatland", "delay0"))
def test_the_condition_changes_what_the_envs_compute(cfg, cond):
    differ = PS.envs_that_differ(PS.reference(cfg, cond).final, PS.reference(cfg, "base").final)
    assert 4 * len(differ) >= 3 * PS.E, (cond, len(differ))
    # (and the schedule was the same: every launch made its decisions)
    assert PS.reference(cfg, cond).outs == PS.reference(cfg, "base").outs == [k * PS.E for k in PS.SCHEDULES[cfg]]


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("cond", ("short", "lr_past"))
def test_the_short_table_is_crossed_inside_a_launch(cfg, cond):
    """Rows past the table's 48 entries are reached in the middle of a long launch (on the oracle, to which the suite
    pins the host build).  For lr_past this is the whole host side: the host build computes the pow and raises nothing
    (sfl_core.h sets the lr-table error in device code only), so its run ends like any other."""
    assert 4 * len(PS.table_crossings(cfg, cond)) >= 3 * 8, PS.table_crossings(cfg, cond)
    assert PS.reference(cfg, cond).outs == [k * PS.E for k in PS.SCHEDULES[cfg]]


@pytest.mark.parametrize("cfg", CFGS)
def test_the_lr_decay_past_the_table_still_changes_the_tables(cfg):
    differ = PS.envs_that_differ(PS.reference(cfg, "lr_past").final, PS.reference(cfg, "short").final)
    assert 4 * len(differ) >= 3 * PS.E, len(differ)


@pytest.mark.parametrize("cfg", CFGS)
def test_no_subgenerator_table_changes_nothing_on_the_host(cfg):
    """The table only saves the sub-generator's run: the host build, which never has it, is the reference of both."""
    assert PS.envs_that_differ(PS.reference(cfg, "notable").final, PS.reference(cfg, "base").final) == []


@pytest.mark.parametrize("cfg", CFGS)
def test_greedy_rounds_between_learning_launches(cfg):
    assert 4 * len(PS.greedy_between_learning(cfg)) >= 3 * PS.E, len(PS.greedy_between_learning(cfg))


@pytest.mark.parametrize("cfg", CFGS)
def test_the_episode_target_and_the_budget_change(cfg):
    """learn(2) ends two episodes per env and learn(3) three, three quarters of them by the cut after 61 decisions; the steps between them make
    57 and 1 decisions per env."""
    first, n57, second, n1 = PS.reference(cfg, "targets").outs
    assert first["decisions"].shape == (2, PS.E) and second["decisions"].shape == (3, PS.E)
    cut = PS.TARGET_MAX_STEPS + 1
    for out in (first, second):  # (a c2 episode can end by itself before the cut)
        assert (out["decisions"] <= cut).all() and 4 * int((out["decisions"] == cut).sum()) >= 3 * out["decisions"].size
    assert (n57, n1) == (57 * PS.E, PS.E)
    assert len({int(x) for x in second["ticks"].ravel()}) > 1  # the envs do not all run alike


@pytest.mark.parametrize("cfg", CFGS)
def test_the_suspension_falls_between_launches_of_both_kinds(cfg):
    sch, at = PS.SCHEDULES[cfg], PS.resume_at(cfg)
    assert 1 in sch[:at] and max(sch[:at]) > 100
    assert 1 in sch[at:] and max(sch[at:]) > 100
    assert sch[at - 1] == sch[at] == 1  # between two one-decision launches


def test_the_groups_differ_in_epsilon_and_in_lr():
    a, b = PS.GROUPS
    assert a["epsilon"] != b["epsilon"] and a["lr"] != b["lr"] and a["lr_decay_rate"] == 1.0 != b["lr_decay_rate"]


# ---- scripts/load_chains.py --counter lgkm ----------------------------------------------------------------------------
KERNEL = "_ZN4sflk8k_wave_gILi16ELi4ELi32ELb0ELi16ELi4ELb0ELb0ELb0ELb0EEEvPKN3sfl6SflMapEPKNS1_8SflStateEPKNS1_6SflCtlE"


def _fragment(*body):
    return [KERNEL + ":\n"] + ["\t" + x + "\n" for x in body] + [".Lfunc_end0:\n"]


def _waits(body, counter="lgkm"):
    return lc.chains(_fragment(*body), counter=counter)[KERNEL]


def test_a_serial_pair_is_two_waits_and_a_batched_pair_one():
    serial = _waits(("s_load_dword s4, s[0:1], 0x0", "s_waitcnt lgkmcnt(0)", "s_load_dword s5, s[0:1], 0x4",
                     "s_waitcnt lgkmcnt(0)"))
    assert [len(ops) for _, _, ops in serial] == [1, 1]
    batched = _waits(("s_load_dword s4, s[0:1], 0x0", "s_load_dword s5, s[0:1], 0x4", "s_waitcnt lgkmcnt(0)"))
    assert [len(ops) for _, _, ops in batched] == [2]
    assert lc.kind_split(serial)["loop"] == {"s": (2, 2)} and lc.kind_split(batched)["loop"] == {"s": (1, 0)}


def test_lds_and_scalar_operations_are_told_apart():
    w = _waits(("ds_read_b32 v1, v0", "ds_bpermute_b32 v2, v0, v1", "s_buffer_load_dword s4, s[0:3], 0x0",
                "s_waitcnt vmcnt(0) lgkmcnt(0)", "ds_write_b32 v0, v1", "s_waitcnt lgkmcnt(0)"))
    assert [[k for k, _ in ops] for _, _, ops in w] == [["d", "d", "s"], ["d"]]
    assert lc.kind_split(w)["loop"] == {"d": (2, 1), "s": (1, 1)}


def test_a_vmcnt_only_wait_retires_nothing():
    w = _waits(("s_load_dwordx2 s[4:5], s[0:1], 0x0", "ds_read_b32 v1, v0", "s_waitcnt vmcnt(0)",
                "global_load_dword v2, v[0:1], off", "s_waitcnt lgkmcnt(1)"))
    assert len(w) == 1 and [k for k, _ in w[0][2]] == ["s", "d"]  # (the global load is no lgkm operation)
    # and the other way round: the default counter sees the global load only, and an lgkmcnt-only wait retires nothing
    v = _waits(("global_load_dword v2, v[0:1], off", "s_load_dword s4, s[0:1], 0x0", "s_waitcnt lgkmcnt(0)",
                "s_waitcnt vmcnt(0)"), counter="vm")
    assert [len(ops) for _, _, ops in v] == [1]


def _r10_fragment():
    import gzip
    with gzip.open(os.path.join(ROOT, "tests", "golden", "r10_v7_listing_fragment.s.gz"), "rt") as f:
        return f.read().splitlines(True)


def test_the_default_result_on_the_r10_listing_fragment_is_unchanged():
    """tests/golden/r10_v7_listing_fragment.s.gz: the memory, LDS and wait instructions of variant 7 (Plain) from the
    listing of the commit before this counter existed; the .vm.json beside it is what that commit's script made of it."""
    import json
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "r10_v7_listing_fragment.vm.json")))
    got = lc.chains(_r10_fragment())
    assert {k: [[ph, w, l] for ph, w, l in v] for k, v in got.items()} == want
    assert lc.chains(_r10_fragment(), counter="vm") == got


def test_the_lgkm_totals_of_the_r10_fragment_are_the_before_listings():
    (w,) = lc.chains(_r10_fragment(), counter="lgkm").values()
    first = _first_kernel(os.path.join(ROOT, "profiles", "r11_v7_lgkm_chains_before.txt"))
    assert (len(w), sum(len(ops) for _, _, ops in w)) == _row(first, "total")[:2] == (185, 339)
    ks = lc.kind_split(w)["loop"]
    assert ks["s"] + ks["d"] == _row(first, "total")[2:]


def _first_kernel(path):
    first = open(path).read().split("\n_ZN", 2)[1]
    assert "k_wave_gILi16ELi4ELi32ELb0ELi16ELi4ELb0E" in first.splitlines()[0]
    return first


def _row(first, phase):
    import re
    m = re.search(rf"^  {phase}\s+exposed waits\s+(\d+)\s+ops\s+(\d+).*scalar\s+(\d+) \(single\s+(\d+)\)\s+LDS\s+(\d+) \(single\s+(\d+)\)",
                  first, re.M)
    return tuple(int(x) for x in m.groups())


def test_the_committed_listings_have_fewer_scalar_waits_in_post_and_decide():
    before = _first_kernel(os.path.join(ROOT, "profiles", "r11_v7_lgkm_chains_before.txt"))
    after = _first_kernel(os.path.join(ROOT, "profiles", "r11_v7_lgkm_chains_after.txt"))
    assert _row(before, "post")[2:4] == (25, 23) and _row(before, "decide")[2:4] == (11, 10)
    assert 2 * _row(after, "post")[2] < _row(before, "post")[2]
    assert _row(after, "decide")[2] < _row(before, "decide")[2]
    # the LDS side is untouched by this change
    assert _row(after, "decide")[4] == _row(before, "decide")[4]
