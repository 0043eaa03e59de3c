"""A history by key on the simulator session (decision D26; tests/history_keys_cases.py): from_key_streams and three append_keys batches against
from_streams over dense ids from a host dict walked in the same order -- n_users, the streams, history_rows, batch_predict and user_recommendations
with users named by string, trim(drop_users=[strings]), evaluate over a train / test pair that shares one dictionary, the identity of the model's column
dictionaries, the check keys and what append_keys refuses."""
import history_keys_cases as K


def test_keyed_history_gives_from_streams_answers(sim_session):
    K.case_keyed_history(sim_session)


def test_evaluate_over_a_shared_dictionary(sim_session):
    K.case_evaluate_over_a_shared_dictionary(sim_session)


def test_column_dictionaries_are_the_identity(sim_session):
    K.case_column_dictionaries_are_the_identity(sim_session)


def test_check_keys_and_refusals(sim_session):
    K.case_check_keys_and_refusals(sim_session)
