"""urcco_dev_rank_metrics / urcco_dev_tree_sum, user_recommendations and evaluate on the MI355X: the problems and the checks of tests/test_sim_eval.py
(tests/eval_ref.py) -- every round boundary of the rank kernel lies inside 256 positions and both levels of the tree sum inside 257 queries, so no larger
shape is needed."""
import pytest

import eval_ref as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stack(gpu_session):
    return E.Stack(gpu_session)


@pytest.mark.parametrize("num", E.NUMS)
def test_metrics_match_the_restatement(gpu_session, num):
    E.check_problem(gpu_session, num)


def test_two_runs_are_identical(gpu_session):
    E.check_repeatable(gpu_session)


def test_alignment_of_the_tree_sum(gpu_session):
    E.check_alignment(gpu_session)


def test_null_pairs(gpu_session):
    E.check_null_pairs(gpu_session)


def test_bad_arguments(gpu_session):
    E.check_bad_arguments(gpu_session)


def test_user_recommendations_against_batch_predict(stack):
    E.check_user_recommendations(stack, on_device=True)
    E.check_user_recommendations_errors(stack)


def test_evaluate_against_the_restatement(stack):
    E.check_evaluate(stack)
