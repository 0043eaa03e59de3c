"""urcco_dev_audience on the host simulator (kernel LOGIC on the CPU) against the numpy restatement of decision D33 (tests/audience_cases.py): counts, user
ids and score bits at the wave, round, term-round, tile and num edges, under ties, exclusions, weights, compaction, several tiles and chunked users;
the arguments.  tests/test_gpu_audience.py runs the same tests on the MI355X."""
import pytest

import audience_cases as A


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: "-".join(map(str, c)))
def test_reference(sim_session, case):
    A.check_case(sim_session, case)


@pytest.mark.parametrize("case", [A.CASES[3], A.CASES[5]], ids=lambda c: "-".join(map(str, c)))
def test_weighted(sim_session, case):
    A.check_case(sim_session, case, weighted=True)


def test_chunks_and_slabs(sim_session):
    A.check_chunks(sim_session)


def test_tiles_under_a_lowered_bound(sim_session):
    A.check_tiles(sim_session)


def test_arguments(sim_session):
    A.check_arguments(sim_session)
