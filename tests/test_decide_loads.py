"""No case of tests/test_decide_loads_gpu.py is vacuous: on the host build (and, for the action masks, the oracle) the
inputs of tests/_decide_loads.py produce the conditions they are named for, each within a stated share of the envs; and
the committed listing of variant 7 has fewer exposed round trips in decide() than the parent's."""
import os
import re

import numpy as np
import pytest

from tests import _decide_loads as D
from tests import _limits as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONDS = sorted({(c.cfg, c.cond) for c in D.CASES})


def _kinds(cfg, cond):
    return D.one_decision_kinds(D.Case(cfg, None, None, cond))


@pytest.mark.parametrize("cfg,cond", CONDS)
def test_one_decision_launches_are_what_the_stream_says(cfg, cond):
    """Every one-decision launch of every env is one of: no draw, one double, one double and one bounded draw."""
    k = _kinds(cfg, cond)
    assert not k.get("other"), k.get("other")
    assert sum(D.ref_of(D.Case(cfg, None, None, cond)).decisions) == sum(D.SCHEDULES[cfg]) * D.E


@pytest.mark.parametrize("cfg", ("c2", "c3"))
def test_base_mixes_exploring_and_greedy_choices_in_every_env(cfg):
    k = _kinds(cfg, "base")
    assert len(k["explore"]) == D.E and len(k["double"]) == D.E and not k.get("none")


@pytest.mark.parametrize("cfg", ("c2", "c3"))
def test_epsilon_one_explores_at_every_decision(cfg):
    k = _kinds(cfg, "eps1")
    assert set(k) == {"explore"} and len(k["explore"]) == D.E


@pytest.mark.parametrize("cfg", ("c2", "c3"))
def test_epsilon_zero_draws_one_double_per_decision(cfg):
    k = _kinds(cfg, "eps0")
    assert set(k) == {"double"} and len(k["double"]) == D.E
    # and over the long launches: has / buf never move (no bounded draw anywhere in the run)
    r = D.ref_of(D.Case(cfg, None, None, "eps0"))
    assert all(np.array_equal(w[:, 4], r.streams[0][:, 4]) for w in r.streams)


@pytest.mark.parametrize("cfg", ("c2", "c3"))
def test_exploring_decisions_with_one_allowed_action(cfg):
    """At epsilon 1 at least half of the sampled envs decide, within their first 60 decisions, at a switch whose only
    allowed action is STOP: the sub-seed draw is consumed and its word ignored."""
    assert 2 * len(D.single_action_envs(cfg)) >= 16, D.single_action_envs(cfg)


@pytest.mark.parametrize("cfg", ("c2", "c3"))
def test_greedy_rounds_between_learning_ones(cfg):
    """In at least three quarters of the envs a one-decision launch falls into a greedy round that has learning
    decisions before and behind it; no stream moves in such a launch."""
    c = D.Case(cfg, None, None, "exploit")
    assert 4 * len(D.greedy_between_learning(c)) >= 3 * D.E, len(D.greedy_between_learning(c))
    assert 4 * len(_kinds(cfg, "exploit")["none"]) >= 3 * D.E


@pytest.mark.parametrize("cfg", ("c2", "c3"))
def test_the_short_table_is_crossed_inside_a_launch(cfg):
    """In at least three quarters of the sampled envs a switch's interaction count passes the table's end during one
    of the long launches."""
    assert 4 * len(D.table_crossings(cfg)) >= 3 * 8, D.table_crossings(cfg)


@pytest.mark.parametrize("cfg", ("c2", "rej"))
def test_the_crafted_streams_reach_a_rejected_draw(cfg):
    """Two envs of every eight (a quarter) start with a stream whose first bounded draw is one of the two rejecting
    sub-seeds, at a decision with three allowed actions: the sub-generator's first word is 0, which Lemire rejects for a
    range of three, and numpy's integers(0, 3) then gives 2."""
    sc = D.compiled(cfg).scenario
    assert D.first_masks(sc, D.SEEDS[0], lm.HP_EXPLORE, 1) == [3]
    states = lm.draw_states(D.SEEDS)
    subs = lm.draw_sub_seeds(D.E)
    rejecting = [e for e in range(D.E) if subs[e] in lm.REJECTING]
    assert 4 * len(rejecting) == D.E
    for e in rejecting[:4]:
        g = lm.numpy_generator(states[e])
        g.random()
        assert int(g.integers(0, lm.SUB_RANGE)) == subs[e]
        sub = np.random.default_rng(subs[e])
        assert int(sub.bit_generator.random_raw() & 0xFFFFFFFF) == 0
        assert int(np.random.default_rng(subs[e]).integers(0, 3)) == 2
    # the first decision of every env explores (epsilon 1) and consumes the crafted buffer
    r = D.ref_of(D.Case(cfg, None, None, "reject"))
    assert all(D.classify(r.streams[0][e], r.streams[1][e]) == "explore" for e in range(D.E))


def test_the_groups_explore_at_different_rates():
    """Group 0 (epsilon 0.9) explores in more than two thirds of its one-decision launches, group 1 (epsilon 0.1,
    decaying faster) in fewer than a fifth: a device that read the wrong group's row cannot match the host build."""
    ex, tot = D.explore_share_by_group(D.Case("c2", None, None, "hpg"))
    assert 3 * ex[0] > 2 * tot[0] and 5 * ex[1] < tot[1], (ex, tot)


def test_variant_7_maps_are_variant_7_shapes():
    for cfg in ("c3", "rej"):
        cm = D.compiled(cfg)
        assert (cm.S, cm.T) == (64, 32), (cfg, cm.S, cm.T)


def _decide_round_trips(path):
    """decide()'s exposed round trips of the first kernel (variant 7, Plain) of a scripts/load_chains.py report."""
    txt = open(path).read()
    first = txt.split("\n_ZN", 2)[1]
    assert "k_wave_gILi16ELi4ELi32ELb0ELi16ELi4ELb0E" in first.splitlines()[0]
    return int(re.search(r"^  decide\s+exposed round trips\s+(\d+)", first, re.M).group(1))


def test_the_committed_listing_has_fewer_round_trips_in_decide():
    parent = _decide_round_trips(os.path.join(ROOT, "profiles", "r09_v7_load_chains_after.txt"))
    new = _decide_round_trips(os.path.join(ROOT, "profiles", "r10_v7_load_chains_after.txt"))
    assert parent == 2 and new < parent, (parent, new)
