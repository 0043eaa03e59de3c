"""The sort + unique row unit (csrc/cco_sorted_rows.h) through urcco_dev_csr_from_pairs on hardware: rows on every class edge, exactly np.unique
per row (sorted_rows_cases.py)."""
import pytest

from sorted_rows_cases import check

pytestmark = pytest.mark.gpu


def test_csr_from_pairs_on_every_class_edge(gpu_session):
    check(gpu_session)
