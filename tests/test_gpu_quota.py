"""urcco_dev_quota_cut on the MI355X: the tests of tests/test_sim_quota.py with the GPU session in the simulator's place -- every round, num, tier and
value-bound edge lies inside 400 rows of at most 256 candidates, so no larger shape is needed."""
import pytest

from test_sim_quota import test_arguments, test_one_value_and_chain, test_walk  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture
def sim_session(gpu_session):
    return gpu_session
