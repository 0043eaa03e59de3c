"""urcco_dev_list_exposure, _exposure_stats and _list_links on the host simulator (kernel LOGIC on the CPU) against the definitions of decision D35
(tests/list_metrics_cases.py), the floats of evaluate.list_metrics and the arguments.  tests/test_gpu_list_metrics.py runs the same tests on the MI355X."""
import pytest

import list_metrics_cases as L


@pytest.mark.parametrize("case", L.CASES + ["zero", "equal"], ids=lambda c: c if isinstance(c, str) else "-".join(map(str, c[:3])))
def test_table(sim_session, case):
    L.check_case(sim_session, case)


@pytest.mark.parametrize("name", sorted(L.BUCKETS))
def test_statistics(sim_session, name):
    L.check_stats(sim_session, L.BUCKETS[name])


def test_links_across_rounds_and_full(sim_session):
    L.check_links(sim_session, L.special())
    assert L.check_links(sim_session, L.full())[:2, 1].tolist() == [256 * 255] * 2


def test_arguments(sim_session):
    L.check_arguments(sim_session)
