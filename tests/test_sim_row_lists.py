"""Every row list of the binning pass in one build (tests/row_lists_cases.py) on the host simulator: at least two rows in each of the 13 lists, against the
oracle, bit for bit against the builds with one launch per class, rows per public bin, and the distinct-candidate count that no row run twice or skipped
leaves intact."""
import row_lists_cases as C


def test_every_row_list_in_one_build(sim_session):
    C.case_every_list(sim_session)
