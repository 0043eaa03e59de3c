"""urcco_dev_recommend on the MI355X against the brute-force restatement of the scoring contract (tests/recommend_ref.py): counts, ids and
scores exact, the class split read from the statistics.  Shapes: the smallest at which the real kernels can go wrong -- more queries than
resident blocks, history rows beyond a wave, a row that overflows the LDS class, item ids and positions beyond 16 bits."""
import itertools

import numpy as np
import pytest

import recommend_ref as R
from universal_recommender_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small():
    # history rows of 0-40 terms plus one row of 600 terms (w = 600 columns x ~10 entries: the global class under the production limit)
    return R.make_problem(21, 3000, 2000, cols=(3000, 5000, 40), boosts=(1.05, 20.0, 0.3), k=20, hist_hi=40, long_row=600)


@pytest.fixture(scope="module")
def small_dev(gpu_session, small):
    return R.DeviceProblem(gpu_session, small)


@pytest.mark.parametrize("num", [1, 20, 256])
def test_every_combination_matches_the_restatement(small_dev, num):
    for use_excl, use_mask, use_fill, no_backfill in itertools.product((False, True), repeat=4):
        stats = R.check(small_dev, num, use_excl, use_mask, use_fill, no_backfill)
        assert stats[0] > 0 and stats[1] >= 1, stats   # (the exact split is asserted by check)


@pytest.mark.parametrize("n_clauses", [0, 1, 16])
def test_clause_counts(small_dev, n_clauses):
    ids = [c % 3 for c in range(n_clauses)]
    boosts = [1.05 + 0.7 * c for c in range(n_clauses)]
    R.check(small_dev, 20, clause_ids=ids, boosts=boosts)
    R.check(small_dev, 20, no_backfill=True, clause_ids=ids, boosts=boosts)


def test_wide_catalogue_and_hub_columns(gpu_session):
    """70 000 items: ids and backfill positions beyond 16 bits.  Three hub columns listed by 90 % of the item rows; half of the 64 queries hold them
    and touch most of the catalogue (the global class, tens of thousands of candidates each: the radix select over a long candidate list)."""
    p = R.make_problem(22, 70_000, 64, cols=(70_000, 5000, 2000), boosts=(1.05, 20.0, 3.0), k=4, hist_hi=10, hub_cols=(5, 77, 40_000), hub_frac=0.9,
                       hub_query_frac=0.5)
    dp = R.DeviceProblem(gpu_session, p)
    for num in (1, 20, 256):
        stats = R.check(dp, num)
        assert 16 <= stats[1] <= 48 and stats[0] + stats[1] == 64
    R.check(dp, 256, use_excl=False, use_mask=False, use_fill=False)
    R.check(dp, 20, no_backfill=True)


def test_ties_at_the_cut_global_class(gpu_session):
    """Every candidate scores 1.05: the cut lies in the position digits alone.  70 000 items, all listed; the winners' positions start at 0, 250 and
    65 530 and straddle the 2^8 and 2^16 boundaries, so the threshold's digits carry across bytes.  w = 70 000, 70 250, 135 530."""
    starts = (0, 250, 65_530)
    p = R.make_tie_problem(24, 70_000, 70_000, starts)
    assert R.work_bound(p, True).tolist() == [70_000, 70_250, 135_530]
    R.check_ties(R.DeviceProblem(gpu_session, p), starts, split=(0, 3))


def test_ties_at_the_cut_lds_class(gpu_session):
    """3 000 items, 2 800 listed: w = 2 800 and 3 050 <= REC_LDS_LIMIT, at most 3 050 of the 4 096 table slots in use.  Once more without fill_order:
    position = item id."""
    starts = (0, 250)
    p = R.make_tie_problem(25, 3000, 2800, starts)
    assert R.work_bound(p, True).tolist() == [2800, 3050] and _lib.REC_LDS_LIMIT == 3072
    dp = R.DeviceProblem(gpu_session, p)
    R.check_ties(dp, starts, split=(2, 0))
    for num in (1, 20, 256):
        stats = R.check(dp, num, use_fill=False)
        assert (int(stats[0]), int(stats[1])) == (2, 0)


def test_reversed_fill_order_half_masked_long_exclusions(gpu_session):
    p = R.make_problem(23, 3000, 500, cols=(3000, 5000, 40), boosts=(1.05, 20.0, 0.3), k=20, hist_hi=40, excl_hi=500, mask_frac=0.5, reverse_fill=True)
    assert np.diff(p.excl_rp).max() >= 400 and 0.4 < p.mask.mean() < 0.6 and p.fill_order[0] == 2999
    dp = R.DeviceProblem(gpu_session, p)
    for num in (1, 20, 256):
        R.check(dp, num)
        R.check(dp, num, no_backfill=True)
