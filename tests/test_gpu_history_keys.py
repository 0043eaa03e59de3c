"""A history by key on hardware (decision D26): the cases of tests/history_keys_cases.py, as tests/test_history_keys_predict.py runs them on the simulator."""
import pytest

import history_keys_cases as K

pytestmark = pytest.mark.gpu


def test_keyed_history_gives_from_streams_answers(gpu_session):
    K.case_keyed_history(gpu_session)


def test_evaluate_over_a_shared_dictionary(gpu_session):
    K.case_evaluate_over_a_shared_dictionary(gpu_session)


def test_column_dictionaries_are_the_identity(gpu_session):
    K.case_column_dictionaries_are_the_identity(gpu_session)


def test_check_keys_and_refusals(gpu_session):
    K.case_check_keys_and_refusals(gpu_session)
