"""urcco_dev_props_compact on the MI355X: the cases of tests/test_sim_props_compact.py (tests/props_compact_cases.py) and D25's larger shape -- 2^20 + 77
property events over 2^16 items with a Zipf(1.2) item distribution, a third of them $unsets, 500 $deletes -- compacted through
properties.DeviceProperties and checked against the numpy restatement."""
import pytest

import props_compact_cases as CC

pytestmark = pytest.mark.gpu


def test_slice_class_edges(gpu_session):
    CC.slice_cases(gpu_session)


def test_copy_tiles(gpu_session):
    CC.tile_cases(gpu_session)


def test_one_item_owns_the_stream(gpu_session):
    CC.owner_case(gpu_session)


def test_every_winner_dead(gpu_session):
    CC.dead_case(gpu_session)


def test_item_and_event_domain(gpu_session):
    CC.domain_cases(gpu_session)


def test_malformed_state_stays_inside_the_arrays(gpu_session):
    CC.malformed_cases(gpu_session)


def test_bad_arguments(gpu_session):
    CC.bad_argument_cases(gpu_session)


def test_compacted_store_and_its_twin(gpu_session):
    CC.twin_case(gpu_session)


def test_compacted_properties_through_batch_predict(gpu_session):
    CC.predict_case(gpu_session)


def test_larger_shape(gpu_session):
    CC.larger_shape_case(gpu_session)
