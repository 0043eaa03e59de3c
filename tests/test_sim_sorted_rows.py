"""The sort + unique row unit (csrc/cco_sorted_rows.h) through urcco_dev_csr_from_pairs on the host simulator: rows on every class edge, exactly
np.unique per row (sorted_rows_cases.py)."""
from sorted_rows_cases import check


def test_csr_from_pairs_on_every_class_edge(sim_session):
    check(sim_session)
