"""urcco_dev_quota_cut on the host simulator (kernel LOGIC on the CPU) against the sequential walk of decision D34 (tests/quota_cases.py): counts, ids,
score bits, `short` and the predictable statistics at the round and num edges, under one to four rules, repeats and items outside the catalogue, in the
LDS tier and -- under a lowered URCCO_QUOTA_LDS_SLOTS -- in the global tier; the arguments.  tests/test_gpu_quota.py runs the same tests on the MI355X."""
import pytest

import quota_cases as Q


@pytest.mark.parametrize("slots", [None, 64], ids=["lds", "global"])
@pytest.mark.parametrize("case", Q.CASES, ids=lambda c: "-".join(map(str, c[:4])) + "-" + "".join(map(str, c[4])))
def test_walk(sim_session, case, slots):
    Q.check_case(sim_session, case, slots)


@pytest.mark.parametrize("slots", [None, 64], ids=["lds", "global"])
def test_one_value_and_chain(sim_session, slots):
    Q.check_rounds(sim_session, slots)


def test_arguments(sim_session):
    Q.check_arguments(sim_session)
