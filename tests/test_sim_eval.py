"""urcco_dev_rank_metrics / urcco_dev_tree_sum on the host simulator (kernel LOGIC on the CPU) against the restatement of decision D19
(tests/eval_ref.py): hits, average precision, NDCG and both sums bit for bit on the planted problem of every table width; repeatability, alignment of the
tree sum, the NULL pairs, URCCO_BAD_ARG; user_recommendations against batch_predict and evaluate against the restatement applied to batch_predict's
answers.  tests/test_gpu_eval.py runs the same checks on the MI355X."""
import os
import subprocess
import sys

import pytest

import eval_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def stack(sim_session):
    return E.Stack(sim_session)


@pytest.mark.parametrize("num", E.NUMS)
def test_metrics_match_the_restatement(sim_session, num):
    p = E.check_problem(sim_session, num)
    assert 120 <= p.n <= 280


def test_problem_sizes():
    assert 600 <= sum(E.problem(num).n for num in E.NUMS) <= 900          # about 700 queries over 5 000 items in all


def test_two_runs_are_identical(sim_session):
    E.check_repeatable(sim_session)


def test_alignment_of_the_tree_sum(sim_session):
    E.check_alignment(sim_session)


def test_null_pairs(sim_session):
    E.check_null_pairs(sim_session)


def test_bad_arguments(sim_session):
    E.check_bad_arguments(sim_session)


def test_user_recommendations_against_batch_predict(stack):
    E.check_user_recommendations(stack, on_device=False)
    E.check_user_recommendations_errors(stack)


def test_evaluate_against_the_restatement(stack):
    E.check_evaluate(stack)


def test_under_guard_pages():
    """The kernel-level tests of this module once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument)."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    env = dict(os.environ, HIPSIM_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "restatement and not evaluate or alignment or null or bad"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
