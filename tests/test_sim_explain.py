"""urcco_dev_explain on the host simulator (kernel LOGIC on the CPU) against the restatement of decision D30 (tests/explain_ref.py): per-clause sums, listed
terms and their order bit for bit at the round, buffer, search, staging and slot edges, two runs each; the score fold against
urcco_dev_recommend_weighted in both of its classes; the arguments.  tests/test_gpu_explain.py runs the same tests on the MI355X."""
import pytest

import explain_ref as X


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: "-".join(map(str, c)))
def test_restatement(sim_session, case):
    X.check(sim_session, *getattr(X, case[0])(*case[1:]))


@pytest.mark.parametrize("weighted", [False, True])
def test_fold_of_the_sums_is_the_recommend_score(sim_session, weighted):
    X.check_score(sim_session, weighted)


def test_arguments(sim_session):
    X.check_arguments(sim_session)
