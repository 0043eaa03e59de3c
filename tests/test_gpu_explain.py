"""urcco_dev_explain on the MI355X: the tests of tests/test_sim_explain.py with the GPU session in the simulator's place -- every round and buffer edge lies
inside 300 matches, the staging switch at 8193 terms and every slot path inside num = 256, so no larger shape is needed."""
import pytest

from test_sim_explain import test_arguments, test_fold_of_the_sums_is_the_recommend_score, test_restatement  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture
def sim_session(gpu_session):
    return gpu_session
