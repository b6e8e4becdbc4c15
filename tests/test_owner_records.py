"""sfl_part_owner on hand-made message segments against the numpy model of tests/_owner.py, on the host build of the
owner step (sfl_part.h part_owner_group, part_update_one, part_answer_one: sfl_core.h row_max / max_action).  The same
cases run on the MI355X in tests/test_owner_records_gpu.py."""
import numpy as np
import pytest

from tests import _owner as ow
from tests import hostsim


def _make(**kw):
    return ow.Owner(hostsim.lib(), **kw)


@pytest.mark.parametrize("name", list(ow.CASES))
def test_owner_case(name):
    ow.CASES[name](_make)


def test_model_rules():
    """The model itself: np.argmax's first maximum, Python's max for the bits of a zero, the masked fallback."""
    b = ow.Blocks(ow.sh.compiled(ow.ROW))
    m = ow.Model(b, 0.0)
    g = ow.wide_port(b)
    cols, na = b.cols[g], b.na[g]
    assert (min(len(c) for c in b.cols.values()), max(len(c) for c in b.cols.values())) == (2, 3)
    assert sorted(set(b.na.values())) == [5, 9] and len(b.ports) == 16
    passes = ow.fill_records(b, 0, g, 0, (-1.0, -0.0, -5e-324), 0.0)
    assert len(passes) == 2
    for p in passes:
        m.group(p)
    row = m.q[(0, g, 0)]
    assert [ow.bits(row[a]) for a in cols] == [ow.bits(x) for x in (-1.0, -0.0, -5e-324)]
    filler = [a for a in range(na) if a not in cols]
    assert filler[0] < cols[0] and filler[-1] > cols[1]
    full = sum(1 << a for a in cols)
    action, mq = m.answer(ow.req(0, g, 0, full))
    # the maximum is a zero: the filler's +0.0 comes first (a lower index), and the mask allows only the stored -0.0
    assert ow.bits(mq) == ow.bits(0.0) and action == cols[1]
    assert m.answer(ow.req(0, g, 0, full, explore=True)) == (-1, mq)
    assert m.answer(ow.req(0, g, 0, 1 << cols[2]))[0] == cols[2]
    assert len(b.masks(g)) == 4 and all((x >> cols[-1]) & 1 for x in b.masks(g))
    assert np.array_equal(m.table(0)[0][b.q_off[g]: b.q_off[g] + 3].view(np.uint64),
                          np.array([-1.0, -0.0, -5e-324]).view(np.uint64))


def test_constants_equal_the_sources():
    import ctypes as C
    _src = ow.src
    assert "constexpr uint32_t PART_UPD_ENV_MAX = %d;" % (ow.PART_GROUP_MAX - 1) in _src("sfl_part.h")
    assert "PART_GROUP_MAX = PART_UPD_ENV_MAX + 1;" in _src("sfl_part.h")
    kinds = "enum : uint32_t { MSG_UPD = 0u, MSG_INSERT = 1u, MSG_VOID = 2u, MSG_REQ = 3u, MSG_REQ_X = 4u };"
    assert kinds in _src("sfl_part.h")
    assert "constexpr int OWN_CHUNK = %d;" % ow.OWN_CHUNK in _src("sfl.hip")
    ms, rp = C.c_uint32(), C.c_uint32()
    assert hostsim.lib().dll.sfl_part_record_sizes(C.byref(ms), C.byref(rp)) == 0
    assert (ms.value, rp.value) == (ow.MSG.itemsize, ow.REP.itemsize)
