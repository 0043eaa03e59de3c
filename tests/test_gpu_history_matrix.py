"""urcco_dev_history_users / urcco_dev_history_matrix on the MI355X: the cases of tests/test_sim_history_matrix.py (tests/history_matrix_cases.py), one
larger shape -- 2^21 + 77 events over 2^17 users with a Zipf user distribution, more than one round of the kernels' grids, all three row classes -- and
URAlgorithm.train_from_history against the build over csr_from_pairs of the same events.  Every device step is one library call."""
import numpy as np
import pytest

import history_matrix_cases as M

pytestmark = pytest.mark.gpu


def test_class_edges(gpu_session):
    M.edge_cases(gpu_session)


def test_window(gpu_session):
    M.window_cases(gpu_session)


def test_users(gpu_session):
    M.user_cases(gpu_session)


def test_several_heavy_rows_per_block(gpu_session):
    M.heavy_rows_case(gpu_session)


def test_capacity(gpu_session):
    M.capacity_cases(gpu_session)


def test_hostile_index(gpu_session):
    M.hostile_cases(gpu_session)


def test_against_csr_from_pairs(gpu_session):
    M.pairs_cases(gpu_session)


def test_bad_arguments(gpu_session):
    M.bad_argument_cases(gpu_session)


def test_larger_shape(gpu_session):
    """2^21 + 77 events over 2^17 users, Zipf(1.3), 2^20 columns: the heaviest user owns more than 100 000 events, at least a quarter of the users none.
    A window that holds about half of the events, min_events 2.  Both calls against the numpy restatement; all three classes are hit."""
    rng = np.random.default_rng(37)
    n, n_users, n_cols = (1 << 21) + 77, 1 << 17, 1 << 20
    users = ((rng.zipf(1.3, n) - 1) % n_users).astype(np.int32)
    users[rng.integers(0, n, 500)] = -1
    cnt = np.bincount(users[users >= 0], minlength=n_users)
    assert cnt.max() > 100_000 and np.count_nonzero(cnt == 0) >= n_users // 4
    times = (M.T0 + rng.integers(-1000, 1000, n)).astype(np.int64)
    t = M.from_users("larger shape", users, n_users, n_cols, rng.integers(-1, n_cols + 1, n), times, rng)
    wave, block, bitmap = M.classes_of(t.rp)
    assert wave > 1000 and block > 100 and bitmap > 10, (wave, block, bitmap)
    row_of, n_rows, rp, ci = M.check(gpu_session, t, (M.T0, M.I64_MAX), 2)
    assert n_users // 8 < n_rows < n_users and n // 4 < rp[-1] < n * 5 // 8 and row_of[int(np.argmax(cnt))] >= 0
    M.check(gpu_session, M.MatProblem("larger shape, untimed", n_users, n_cols, t.items, None, t.rp, t.pos))


def test_train_from_history(gpu_session):
    """A history that was appended to and trimmed, retrained in a window: the indicator matrices are those of the build over csr_from_pairs of the same
    events, bit for bit, and batch_predict over the two models agrees"""
    M.check_train_from_history(gpu_session, 3000, 400, 250, 200)
