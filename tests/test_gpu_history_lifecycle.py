"""DeviceHistory over its life on the MI355X: the schedules of tests/history_lifecycle_cases.py at their full size -- a user beyond the matrix
kernel's LDS row limit included -- with the object compared after every step against a host model in numpy (tests/test_sim_history_lifecycle.py
describes the checks).  Every device step is one library call on the object's live tensors."""
import pytest

import history_lifecycle_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stack(gpu_session):
    return L.stack_for(gpu_session)


def test_dense_schedule(gpu_session, stack):
    L.run(gpu_session, stack, L.make_dense_schedule())


def test_keyed_schedule(gpu_session, stack):
    L.run(gpu_session, stack, L.make_keyed_schedule())


def test_dense_schedule_twice(gpu_session, stack):
    """two fresh objects through the dense schedule: all streams, idx_row_ptr, history rows, matrices and ranks bit for bit"""
    a = L.run(gpu_session, stack, L.make_dense_schedule(), check=False)
    b = L.run(gpu_session, stack, L.make_dense_schedule(), check=False)
    assert len(a) == len(b) > 8 and L.same_trace(a, b)
