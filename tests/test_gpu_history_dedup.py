"""urcco_dev_history_dedup on the MI355X: the cases of tests/test_sim_history_dedup.py (tests/history_dedup_cases.py) and one larger shape -- 2^20 + 77
events over 2^16 users with Zipf user and item distributions.  Every device step is one library call."""
import pytest

import history_dedup_cases as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("keep", sorted(D.KEEPS))
@pytest.mark.parametrize("case", D.CASES + [(D.larger_shape_case, ())], ids=D.IDS + ["larger_shape_case"])
def test_dedup(gpu_session, case, keep):
    case[0](gpu_session, keep, *case[1])
