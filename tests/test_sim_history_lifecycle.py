"""DeviceHistory over its life on the host simulator (kernel LOGIC on the CPU): the two schedules of tests/history_lifecycle_cases.py -- about a dozen
interleaved appends and trims on ONE object -- with the object compared after every step against a host model in numpy: the streams and their indexes,
the history rows at caps below, at and above the planted counts, on three steps matrices and ranks, on two batch_predict against the dict form, and
at the end the buffer contract.  The shapes are those of tests/test_gpu_history_lifecycle.py: the simulator takes a few seconds for them, no
assertion on the shapes is dropped here.  The rerun under HIPSIM_GUARD ends every tensor of the session's allocator -- the object's buffers with
their spare capacity among them -- at a PROT_NONE page."""
import os
import subprocess
import sys

import pytest

import history_lifecycle_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def stack(sim_session):
    return L.stack_for(sim_session)


def test_every_step_of_the_schedules_is_needed():
    """Host model only.  Both schedules pass assert_schedule; with any single step taken out it raises: no step can leave quietly."""
    for make in (L.make_dense_schedule, L.make_keyed_schedule):
        s = make()
        L.assert_schedule(s)
        for k in range(len(s.steps)):
            with pytest.raises(AssertionError):
                L.assert_schedule(L.Schedule(s.keyed, s.steps[:k] + s.steps[k + 1:], s.planted, s.n_users_max))


def test_dense_schedule(sim_session, stack):
    L.run(sim_session, stack, L.make_dense_schedule())


def test_keyed_schedule(sim_session, stack):
    L.run(sim_session, stack, L.make_keyed_schedule())


def test_dense_schedule_twice(sim_session, stack):
    """two fresh objects through the dense schedule: all streams, idx_row_ptr, history rows, matrices and ranks bit for bit"""
    a = L.run(sim_session, stack, L.make_dense_schedule(), check=False)
    b = L.run(sim_session, stack, L.make_dense_schedule(), check=False)
    assert len(a) == len(b) > 8 and L.same_trace(a, b)


def test_under_guard_pages():
    """This module once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument)."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    env = dict(os.environ, HIPSIM_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
