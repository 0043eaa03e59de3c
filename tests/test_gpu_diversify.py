"""urcco_dev_diversify on the MI355X: the tests of tests/test_sim_diversify.py with the GPU session in the simulator's place -- every lane-slot, bitmap-word
and num edge lies inside 256 candidates; the 3300-row table outnumbers the waves of the grid, so the row loop strides here too."""
import pytest

from test_sim_diversify import test_arguments, test_constructed, test_rule  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture
def sim_session(gpu_session):
    return gpu_session
