"""k_part_owner (sfl.hip: its chunks and tails, its stage loop, part_answer_fast's own copy of row_max / max_action) on
the MI355X against the numpy model of tests/_owner.py, record by record: the cases of tests/test_owner_records.py with
the message and reply buffers as device tensors."""
import importlib

import pytest

from tests import _owner as ow

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("network-distributed-q-learning_amd._lib")
build = importlib.import_module("network-distributed-q-learning_amd.build")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_product()


@pytest.mark.parametrize("name", list(ow.CASES))
def test_owner_case(lib, name):
    ow.CASES[name](lambda **kw: ow.Owner(lib, device="cuda", **kw))
