"""The list metrics of decision D35 on the MI355X: the tests of tests/test_sim_list_metrics.py with the GPU session in the simulator's place."""
import pytest

from test_sim_list_metrics import test_arguments, test_links_across_rounds_and_full, test_statistics, test_table  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture
def sim_session(gpu_session):
    return gpu_session
