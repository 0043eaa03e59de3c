"""The host level's boundary check on hardware: the in-range cases of tests/boundary_check_cases.py (a decreasing pair, a duplicate) at the device's own
CU count -- the row counts follow from it, so that every geometry has a second grid round -- plus everything planted at once, a violation in a secondary
event type, and the false-positive control.  Out-of-range columns and corrupt row_ptr entries stay on the simulator on purpose: if the check had a hole
there, the build behind it would run with an out-of-bounds index; a missed in-range violation merely inflates counts, and it exercises the same lanes
and positions."""
import pytest
import torch

import boundary_check_cases as B

pytestmark = pytest.mark.gpu
GS = (2, 8, 64)


@pytest.fixture(scope="module")
def host_lib(gpu_session):
    try:
        yield gpu_session.lib
    finally:
        gpu_session.lib.urcco_shutdown()


@pytest.fixture(scope="module")
def n_cu(gpu_session):
    return torch.cuda.get_device_properties(gpu_session.device).multi_processor_count


IN_RANGE = [(G, kind, place, t) for G in GS for kind in B.KINDS for place in B.PLACES for t in B.offsets(G)]


@pytest.mark.parametrize("G,kind,place,t", IN_RANGE, ids=["G{}-{}-{}-t{}".format(*c) for c in IN_RANGE])
def test_in_range_violation_is_counted_once(host_lib, n_cu, G, kind, place, t):
    B.case_in_range(host_lib, n_cu, G, kind, place, t)


@pytest.mark.parametrize("G", GS)
def test_all_planted_at_once(host_lib, n_cu, G):
    assert B.case_all_at_once(host_lib, n_cu, G) >= 16


@pytest.mark.parametrize("bad_dataset", [1, 2])
def test_violation_in_a_secondary(host_lib, n_cu, bad_dataset):
    B.case_secondary(host_lib, n_cu, bad_dataset)


@pytest.mark.parametrize("G", [2, 8])
def test_control_first_column_below_the_previous_row_s_last(host_lib, G):
    B.case_first_column_below_previous_last(host_lib, G)
