"""The sender side of a partitioned round on the host build (sfl_part.h env_run_part, sfl_hostsim.cpp part_compact),
many ranks in one process, against the order-independent segment model of tests/_segments.py; the model's own
self-checks (each mutation of a captured buffer makes it fail); and the exact deferral model: the host build's
compaction runs in env order, so a first-come count says who is deferred in every round.  The same cases run on the
MI355X in tests/test_segments_gpu.py."""
import pytest

from tests import _segments as sg
from tests import hostsim

SLOW = {"w8-e600-switch"}  # (over 10 s: the end state of 4,800 envs on 8 ranks)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name, marks=[pytest.mark.slow] if c.name in SLOW else [])
                                  for c in sg.CASES])
def test_case(case):
    got = sg.run_case(case, hostsim.lib())
    assert got["variants"] == [0]


def test_cases_cover_what_the_sweep_is_for():
    """The (ranks, envs per rank) pairs, both owner maps, both local-row settings, a k below, at and above 16 and 17, a
    count read every third round, a change of k within a step, and each purpose in some case."""
    cs = sg.CASES
    assert {(c.W, c.e_loc) for c in cs} == {(1, 257), (2, 64), (5, 257), (8, 300), (8, 600), (3, 1)}
    assert {c.owner for c in cs} == {"part", "rr"} and {c.local for c in cs} == {False, True}
    ks = {k for c in cs for k in c.ks}
    assert {"peak", "peak-1", 17, 16, 3, 1} <= ks
    assert any(c.every == 3 for c in cs) and any(c.switch for c in cs)
    assert {w for c in cs for w in c.want} == {"blocks", "fanout", "two_slot", "episode", "stuck"}
    for c in cs:
        if "blocks" in c.want:
            assert c.e_loc > sg.COMPACT_BLOCK and c.e_loc % sg.COMPACT_BLOCK
    assert "#define SFL_COMPACT_BLOCK %d " % sg.COMPACT_BLOCK in open(sg.ow.CSRC + "/sfl.hip").read()
    assert sg.variant_of(sg.CASE["w2-e64-two-slot"]) == 5 and sg.variant_of(sg.CASE["w2-e64"]) == 1


@pytest.fixture(scope="module")
def captured():
    """A run with deferrals (2 ranks x 64 envs, k = 17) and its twin."""
    case = sg.CASE["w2-e64"]
    cm = sg.compiled(case.map)
    owner = sg.owner_map(cm, case.W, case.owner)
    twin = sg.Twin(sg.run_job(case, hostsim.lib())[0], owner, case.e_loc)
    steps = sg.run_job(case, hostsim.lib(), k=17)[0]
    return case, owner, twin, steps


def _round_with_groups(steps):
    """A round of step 0 with a deferred env, a group of two or more records and a group of one."""
    for i, rnd in enumerate(steps[0]):
        try:
            sg._find(rnd, 2)
            sg.mut_wrong_destination(rnd)
        except AssertionError:
            continue
        if any(c[2 * len(rnd.segs) + 1] for c in rnd.counts):
            return i
    raise AssertionError("no such round")


def test_captured_run_passes(captured):
    case, owner, twin, steps = captured
    st = sg.check_run(steps, twin, env_order=True)
    assert st["deferrals"] > 0 and st["over"] > 0


@pytest.mark.parametrize("name", list(sg.MUTATIONS))
def test_mutation_is_caught(captured, name):
    """Each corruption of one captured round fails A, B or C."""
    case, owner, twin, steps = captured
    i = _round_with_groups(steps)
    bad = [list(s) for s in steps]
    bad[0][i] = sg.MUTATIONS[name](steps[0][i])
    with pytest.raises(sg.SegmentError):
        sg.check_run(bad, twin, env_order=True)
    if name == "drop_group":  # every segment still well formed: B and C alone catch it
        sg.round_sets(bad[0][i], owner, case.e_loc)
    else:
        with pytest.raises(sg.SegmentError):
            sg.round_sets(bad[0][i], owner, case.e_loc)


@pytest.mark.parametrize("field,delta", [("msg", 1), ("peak", 1), ("open", -1), ("defer", 1), ("defer_sum", 1),
                                         ("reqs", 1)])
def test_wrong_count_is_caught(captured, field, delta):
    """C: one count of one rank off by one in one round."""
    case, owner, twin, steps = captured
    W = case.W
    i = _round_with_groups(steps)
    rnd = steps[0][i]
    counts, reqs = [list(c) for c in rnd.counts], list(rnd.reqs)
    if field == "reqs":
        reqs[1] += delta
    else:
        counts[1][dict(msg=0, peak=W, open=2 * W, defer=2 * W + 1, defer_sum=2 * W + 2)[field]] += delta
    bad = [list(s) for s in steps]
    bad[0][i] = sg.Round(rnd.k, rnd.segs, reqs, counts)
    with pytest.raises(sg.SegmentError):
        sg.check_run(bad, twin, env_order=True)
