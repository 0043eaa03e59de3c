"""urcco_dev_audience on the MI355X: the tests of tests/test_sim_audience.py with the GPU session in the simulator's place -- every wave, round, tile and
compaction edge lies inside 4 500 users and 130 query items, so no larger shape is needed."""
import pytest

from test_sim_audience import test_arguments, test_chunks_and_slabs, test_reference, test_tiles_under_a_lowered_bound, test_weighted  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture
def sim_session(gpu_session):
    return gpu_session
