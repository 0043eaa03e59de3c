"""urcco_dev_recommend on the host simulator (kernel LOGIC on the CPU): every combination of exclusions / item mask / fill_order / NO_BACKFILL
against the brute-force restatement of the scoring contract (tests/recommend_ref.py), exact in counts, ids and scores."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recommend_ref as R
from universal_recommender_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_LIMIT = 256   # URCCO_REC_LDS_LIMIT for the hub run: at 300 items a hub column is 300 touches, far below the production limit


@pytest.fixture(scope="module")
def problem():
    # 300 items, 200 queries, clauses over 300 / 500 / 7 columns, indicator rows of <= 10 entries, history rows of 0-30 terms, one hub column (column 0
    # of the first clause) listed by every item row; boosts that are not dyadic
    return R.make_problem(11, 300, 200, cols=(300, 500, 7), boosts=(1.05, 20.0, 0.3), k=10, hist_hi=30, hub_cols=(0,), hub_frac=1.0, hub_query_frac=0.25)


@pytest.fixture(scope="module")
def dev(sim_session, problem):
    return R.DeviceProblem(sim_session, problem)


@pytest.fixture()
def low_limit():
    os.environ["URCCO_REC_LDS_LIMIT"] = str(SIM_LIMIT)
    yield SIM_LIMIT
    del os.environ["URCCO_REC_LDS_LIMIT"]


@pytest.mark.parametrize("num", [1, 4, 20])
def test_every_combination_matches_the_restatement(dev, num, low_limit):
    """Hub queries land in the global class, the rest in the LDS class: both classes serve queries in every run."""
    for use_excl, use_mask, use_fill, no_backfill in itertools.product((False, True), repeat=4):
        stats = R.check(dev, num, use_excl, use_mask, use_fill, no_backfill, lds_limit=low_limit)
        assert stats[2] == 0 and stats[0] > 0 and stats[1] > 0, stats


def test_production_limit_keeps_small_queries_in_the_lds_class(dev):
    """The same problem under the production limit: everything fits the LDS table (hub columns included: 300 touches)."""
    stats = R.check(dev, 20)
    assert stats[0] == dev.n_queries and stats[1] == 0


def test_problem_holds_the_edge_cases(problem):
    p = problem
    terms = sum(np.diff(c.q_rp) for c in p.clauses)
    assert (terms == 0).any(), "queries with no terms at all"
    eligible = np.array([np.count_nonzero(np.delete(p.mask, p.excl_ci[p.excl_rp[q]:p.excl_rp[q + 1]])) for q in range(p.n_queries)])
    assert (eligible < 4).any() and (eligible == 0).any(), "queries with fewer eligible items than num"
    s = R.scores_of(p, np.arange(p.n_queries))
    s[:, p.mask == 0] = -1
    assert any(int(np.argmax(s[q])) in p.excl_ci[p.excl_rp[q]:p.excl_rp[q + 1]] and s[q].max() > 0 for q in range(p.n_queries)), "strongest candidate excluded"
    assert np.bincount(p.clauses[0].ind_ci, minlength=300)[0] == 300, "hub column listed by every item row"


@pytest.mark.parametrize("n_clauses", [0, 1, 16])
def test_clause_counts(dev, n_clauses, low_limit):
    ids = [c % 3 for c in range(n_clauses)]
    boosts = [1.05 + 0.7 * c for c in range(n_clauses)]
    R.check(dev, 20, clause_ids=ids, boosts=boosts, lds_limit=low_limit)
    R.check(dev, 4, no_backfill=True, clause_ids=ids, boosts=boosts, lds_limit=low_limit)


def test_largest_num_and_more_than_the_catalogue(dev, low_limit):
    R.check(dev, 256, lds_limit=low_limit)            # most queries have fewer than 256 positives: the backfill completes them
    R.check(dev, 256, use_excl=False, use_mask=False, use_fill=False, lds_limit=low_limit)


TIE_STARTS = (0, 250)


@pytest.fixture(scope="module")
def tie_dev(sim_session):
    # every candidate scores 1.05: the cut lies in the position digits alone.  3 000 items, 2 800 listed: w = 2 800 and 3 050
    p = R.make_tie_problem(25, 3000, 2800, TIE_STARTS)
    assert R.work_bound(p, True).tolist() == [2800, 3050]
    return R.DeviceProblem(sim_session, p)


def test_ties_at_the_cut_lds_class(tie_dev):
    """Under the production limit both queries fit the LDS table (at most 3 050 of its 4 096 slots); once more without fill_order: position = item id."""
    R.check_ties(tie_dev, TIE_STARTS, split=(2, 0))
    stats = R.check(tie_dev, 20, use_fill=False)
    assert (int(stats[0]), int(stats[1])) == (2, 0)


def test_ties_at_the_cut_global_class(tie_dev, low_limit):
    """The same queries under the lowered limit: the global class."""
    R.check_ties(tie_dev, TIE_STARTS, split=(0, 2), lds_limit=low_limit)
    stats = R.check(tie_dev, 20, use_fill=False, lds_limit=low_limit)
    assert (int(stats[0]), int(stats[1])) == (0, 2)


def test_ties_at_the_cut_wide_catalogue(sim_session):
    """70 000 items, all listed (the global class under the production limit): the winners' positions start at 0, 250 and 65 530 and straddle the 2^8 and
    2^16 boundaries, so the threshold's digits carry across bytes."""
    starts = (0, 250, 65_530)
    p = R.make_tie_problem(24, 70_000, 70_000, starts)
    assert R.work_bound(p, True).tolist() == [70_000, 70_250, 135_530]
    R.check_ties(R.DeviceProblem(sim_session, p), starts, split=(0, 3))


def test_bad_arguments(dev):
    s = dev.sess
    ok = dev.clauses

    def status(**kw):
        args = dict(n_queries=dev.n_queries, n_items=dev.p.n_items, clauses=ok, num=4)
        args.update(kw)
        with pytest.raises(_lib.UrccoError) as ei:
            s.recommend(**args)
        return ei.value.status

    assert status(num=0) == _lib.BAD_ARG
    assert status(num=257) == _lib.BAD_ARG
    assert status(clauses=[ok[c % 3] for c in range(17)]) == _lib.BAD_ARG
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert status(clauses=[(ok[0][0], bad) + tuple(ok[0][2:])]) == _lib.BAD_ARG
    arr = (_lib.RecClause * 1)()
    out = torch.zeros(dev.n_queries * 4, dtype=torch.int32)
    sc = torch.zeros(dev.n_queries * 4, dtype=torch.float64)
    for rp, ci in ((dev.excl[0].data_ptr(), None), (None, dev.excl[1].data_ptr())):   # a half-NULL exclusion pair
        assert s.lib.urcco_dev_recommend(s.handle, dev.n_queries, dev.p.n_items, arr, 0, rp, ci, None, None, 4, 0, out.data_ptr(), out.data_ptr(),
                                         sc.data_ptr(), None) == _lib.BAD_ARG


def test_under_guard_pages():
    """This module once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument)."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    env = dict(os.environ, HIPSIM_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
