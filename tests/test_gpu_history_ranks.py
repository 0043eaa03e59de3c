"""urcco_dev_history_ranks / urcco_dev_fill_order on the MI355X: the cases of tests/test_sim_history_ranks.py (tests/history_ranks_cases.py) and one
larger shape each -- 2^21 + 77 events in two streams over 2^16 columns with a Zipf item distribution and a column map that drops a tenth of the columns
and merges some (more than one round of the counting grid, hot items through the block caches), and 2^20 + 3 items sorted by four fields."""
import numpy as np
import pytest

import history_ranks_cases as R

pytestmark = pytest.mark.gpu


def test_interval_bounds(gpu_session):
    R.boundary_cases(gpu_session)


def test_open_window_and_no_end(gpu_session):
    R.open_window_cases(gpu_session)


def test_ids_and_column_maps(gpu_session):
    R.id_cases(gpu_session)


def test_streams(gpu_session):
    R.stream_cases(gpu_session)


def test_block_cache_paths(gpu_session):
    R.cache_cases(gpu_session)


def test_rank_bad_arguments(gpu_session):
    R.rank_bad_argument_cases(gpu_session)


def test_fill_order_sizes(gpu_session):
    R.fill_size_cases(gpu_session)


def test_fill_order_digit_skip(gpu_session):
    R.fill_digit_cases(gpu_session)


def test_fill_order_stability_and_fields(gpu_session):
    R.fill_stability_cases(gpu_session)


def test_fill_order_bad_arguments(gpu_session):
    R.fill_bad_argument_cases(gpu_session)


def test_one_field_is_the_order_of_from_indicators(gpu_session):
    R.from_indicators_case(gpu_session)


def test_larger_counting_shape(gpu_session):
    """2^21 + 77 events in two streams over 2^16 columns, Zipf(1.2): the hottest column takes more than 100 000 events.  The first stream maps its columns
    onto 50 000 items -- a tenth dropped, the rest folded so that items share columns -- the second counts straight into the item table, ids beyond it
    dropped.  All three types against numpy, counts included."""
    rng = np.random.default_rng(41)
    n, n_cols, n_items = (1 << 21) + 77, 1 << 16, 50_000
    cols = ((rng.zipf(1.2, n) - 1) % n_cols).astype(np.int32)
    cols[rng.integers(0, n, 300)] = np.array([-1, n_cols, R.I32_MIN, R.I32_MAX], np.int32)[rng.integers(0, 4, 300)]
    assert np.bincount(cols[(cols >= 0) & (cols < n_cols)]).max() > 100_000
    times = (R.T0 + rng.integers(-100, 3700, n)).astype(np.int64)
    cmap = (rng.permutation(n_cols) % n_items).astype(np.int32)
    cmap[rng.random(n_cols) < 0.1] = -1
    assert np.unique(cmap[cmap >= 0]).size < np.count_nonzero(cmap >= 0)
    at = n // 2 + 13
    streams = [R.RStream(cols[:at], times[:at], cmap, n_cols), R.RStream(cols[at:], times[at:], None, n_cols)]
    for rtype in (R.POPULAR, R.TRENDING, R.HOT):
        rank, counts = R.check_ranks(gpu_session, "larger shape", streams, n_items, rtype, (R.T0, R.T0 + 3600))
        assert n * 19 // 20 > counts.sum() > n // 2 and np.count_nonzero(rank != R.NONE) > 1000
    assert (rank[rank != R.NONE] < 0).any() and (rank > 0).any()


def test_larger_fill_order(gpu_session):
    """2^20 + 3 items, four fields: two that tie heavily, a hot-like field with negative values and items without a rank, counts that decide the rest"""
    rng = np.random.default_rng(43)
    n = (1 << 20) + 3
    fields = [rng.integers(0, 4, n), np.where(rng.random(n) < 0.4, R.NONE, rng.integers(-50, 50, n)), rng.integers(0, 2, n), (rng.zipf(1.3, n) % 100_000).astype(np.int64)]
    R.check_fill(gpu_session, "larger shape", fields, n)
