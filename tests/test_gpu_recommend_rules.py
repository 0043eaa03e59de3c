"""urcco_dev_recommend_rules on the MI355X against the brute force of tests/recommend_rules_ref.py: counts, ids, score bits and stats[0..4]
exact.  Shapes: test_gpu_recommend.py's -- more queries than resident blocks, one history row that overflows the LDS class, item ids and
backfill positions beyond 16 bits under a rule, tens of thousands of candidates of which a NONE rule rejects half."""
import numpy as np
import pytest

import recommend_ref as R
import recommend_rules_ref as RR
from universal_recommender_amd import _lib

pytestmark = pytest.mark.gpu

RULE_SETS = [("any",), ("none",), ("range",), ("ind",), ("any", "none", "range", "ind")]


@pytest.fixture(scope="module")
def small(gpu_session):
    # 3 000 items x 2 000 queries, history rows of 0-40 terms plus one row of 600 terms (the global class under the production limit)
    p = R.make_problem(21, 3000, 2000, cols=(3000, 5000, 40), boosts=(1.05, 20.0, 0.3), k=20, hist_hi=40, long_row=600)
    rules = RR.make_rules(p, 5)
    RR.assert_edge_cases(p, rules)
    return RR.DeviceRules(R.DeviceProblem(gpu_session, p), rules)


@pytest.mark.parametrize("names", RULE_SETS, ids="+".join)
@pytest.mark.parametrize("num", [1, 20, 256])
def test_rule_sets_match_the_restatement(small, names, num):
    for no_backfill in (False, True):
        stats = RR.check(small, names, num, no_backfill=no_backfill)
        assert stats[0] > 0 and stats[1] >= 1, stats
        assert (stats[4] == 0) == no_backfill, stats


def test_no_rules_is_the_rule_free_call(small):
    plain, empty = small.run(None, 20), small.run((), 20)
    live = np.arange(20)[None, :] < plain[0][:, None]
    assert np.array_equal(plain[0], empty[0]) and np.array_equal(plain[1][live], empty[1][live])
    assert np.array_equal(plain[2][live].view(np.int64), empty[2][live].view(np.int64)) and np.array_equal(plain[3], empty[3])
    RR.check(small, [RULE_SETS[-1][j % 4] for j in range(16)], 20)


def test_wide_catalogue_and_hub_columns(gpu_session):
    """70 000 items, three hub columns listed by 90 % of the item rows, half of the 64 queries hold them (the global class, tens of thousands of
    candidates each).  The NONE rule here is made for this shape: every hub query names value 0, which about 60 % of the items hold, so the rule
    turns more than half of those candidates into tombstones; ids and backfill positions beyond 16 bits are walked under the rules."""
    p = R.make_problem(22, 70_000, 64, cols=(70_000, 5000, 2000), boosts=(1.05, 20.0, 3.0), k=4, hist_hi=10, hub_cols=(5, 77, 40_000), hub_frac=0.9,
                       hub_query_frac=0.5)
    rules = RR.make_rules(p, 5)
    RR.assert_edge_cases(p, rules)
    hub = np.array([5 in p.clauses[0].q_ci[p.clauses[0].q_rp[q]:p.clauses[0].q_rp[q + 1]] for q in range(64)])
    none = rules["none"]
    rows = [np.union1d(none.q_ci[none.q_rp[q]:none.q_rp[q + 1]], [0]) if hub[q] else none.q_ci[none.q_rp[q]:none.q_rp[q + 1]] for q in range(64)]
    q_rp, q_ci = R._rows_to_csr(rows)
    rules["none0"] = RR.Rule(_lib.RULE_NONE, none.n_cols, none.m_rp, none.m_ci, q_rp, q_ci)
    rules["none0"].ok = RR._eligibility(p, rules["none0"])
    score = R.scores_of(p, np.arange(64))
    touched = (score > 0) & (p.mask != 0)
    assert hub.sum() >= 16 and (touched[hub].sum(1) > 20_000).all() and ((touched & ~rules["none0"].ok)[hub].sum(1) > 0.5 * touched[hub].sum(1)).all()
    dr = RR.DeviceRules(R.DeviceProblem(gpu_session, p), rules)
    for num in (1, 20, 256):
        stats = RR.check(dr, ("none0",), num)
        assert 16 <= stats[1] <= 48 and stats[0] + stats[1] == 64
    got = dr.run(("any", "none0", "range"), 256)
    assert (got[1][np.arange(256)[None, :] < got[0][:, None]] > 65_535).any(), "ids beyond 16 bits returned under rules"
    RR.check(dr, ("any", "none0", "range"), 256)
    RR.check(dr, ("any", "none0", "range", "ind"), 20)
    RR.check(dr, ("none0", "range"), 20, no_backfill=True)
    RR.check(dr, ("range",), 256, use_excl=False, use_mask=False, use_fill=False)
