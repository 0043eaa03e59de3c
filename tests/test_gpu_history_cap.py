"""urcco_dev_history_cap on the MI355X: the cases of tests/test_sim_history_cap.py (tests/history_cap_cases.py) and one larger shape -- 2^20 + 77
events over 2^16 users with a Zipf user distribution.  Every device step is one library call."""
import pytest

import history_cap_cases as C

pytestmark = pytest.mark.gpu


def test_segment_lengths_and_caps(gpu_session):
    C.segment_cases(gpu_session)


def test_times(gpu_session):
    C.time_cases(gpu_session)


def test_one_user_owns_the_stream(gpu_session):
    C.big_owner_case(gpu_session)


def test_index_order(gpu_session):
    C.index_order_case(gpu_session)


def test_no_cap_is_the_trim(gpu_session):
    C.no_cap_cases(gpu_session)


def test_rules_are_independent(gpu_session):
    C.independence_case(gpu_session)


def test_degenerate_input(gpu_session):
    C.degenerate_cases(gpu_session)


def test_hostile_index(gpu_session):
    C.hostile_cases(gpu_session)


def test_bad_arguments(gpu_session):
    C.bad_argument_cases(gpu_session)


def test_rows_below_the_cap_are_unchanged(gpu_session):
    C.rows_unchanged_case(gpu_session)


def test_capped_history_through_batch_predict(gpu_session):
    C.predict_case(gpu_session)


def test_schedule_on_one_history(gpu_session):
    C.schedule_case(gpu_session)


def test_larger_shape(gpu_session):
    C.larger_shape_case(gpu_session)
