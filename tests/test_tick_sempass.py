"""The cases of tests/test_tick_sempass_gpu.py are not vacuous: on the host build alone, every env of every case ends
at least two episodes, some episode ends at max_episode_steps with trains still on the map, and some train arrives
before a launch boundary behind which its episode ticks on."""
import pytest

from tests import _sempass as S


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_the_reference_goes_through_what_the_case_is_for(c):
    S.check_reference(c)


def test_the_cases_cover_the_shapes():
    assert {(c.cfg, c.G) for c in S.CASES} >= {("c3", 16), ("c3", 64), ("c2", 8), ("c2", 16), ("c2", 32)}
    for c in S.CASES:
        assert 1 in c.schedule and max(c.schedule) >= 100
