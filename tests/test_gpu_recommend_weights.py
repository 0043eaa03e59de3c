"""urcco_dev_recommend_weighted and urcco_dev_idf_weights on the MI355X against the restatement of decision D20 (tests/recommend_weights_ref.py): counts,
ids, score bits and stats[0..4] exact.  Shapes: test_gpu_recommend_rules.py's two problems (more queries than resident blocks with one history row that
overflows the LDS class; 70 000 items with hub columns: tens of thousands of 64-bit counters per query), the two counter bounds of the contract -- a
32-bit LDS counter at 3 072 * 2^20 > 2^31 and a 64-bit global one beyond 2^32 -- and ties between different term sets in both classes."""
import numpy as np
import pytest

import recommend_ref as R
import recommend_rules_ref as RR
import recommend_weights_ref as W
from universal_recommender_amd import _lib

pytestmark = pytest.mark.gpu

ALL_RULES = ("any", "none", "range", "ind")


def device_idf(sess, p: R.Problem, dp: R.DeviceProblem):
    """per clause the idf weights computed by the device (n_docs = the items whose row is not empty), checked against numpy to one unit, read back"""
    out = []
    for cl, dcl in zip(p.clauses, dp.clauses):
        n_docs = int(np.count_nonzero(np.diff(cl.ind_rp)))
        t = sess.idf_weights(dcl[2], cl.n_cols, n_docs)
        sess.synchronize()
        out.append(t.cpu().numpy().copy())
        cp = np.concatenate([[0], np.cumsum(np.bincount(cl.ind_ci, minlength=cl.n_cols))])
        diff = np.abs(out[-1].astype(np.int64) - W.idf_ref(cp, n_docs).astype(np.int64))
        print(f"idf: {cl.n_cols} columns, n_docs {n_docs}, weights {out[-1].min()}..{out[-1].max()}, off by one unit at {int((diff == 1).sum())} columns, max {diff.max()}")
        assert diff.max() <= 1
    return out


@pytest.fixture(scope="module")
def small(gpu_session):
    # 3 000 items x 2 000 queries, history rows of 0-40 terms plus one row of 600 terms (the global class under the production limit)
    p = R.make_problem(21, 3000, 2000, cols=(3000, 5000, 40), boosts=(1.05, 20.0, 0.3), k=20, hist_hi=40, long_row=600)
    rules = RR.make_rules(p, 5)
    dp = R.DeviceProblem(gpu_session, p)
    w = W.random_weights(p, 41, without=(1,))
    assert W.extremes_hit(p, w)
    return W.DeviceWeighted(dp, W.Weighted(p, w), RR.DeviceRules(dp, rules))


@pytest.mark.parametrize("names", [(), ALL_RULES], ids=["plain", "rules"])
@pytest.mark.parametrize("num", [1, 20, 256])
def test_random_weights_match_the_restatement(small, names, num):
    for no_backfill in (False, True):
        stats = W.check(small, names, num, no_backfill=no_backfill)
        assert stats[0] > 0 and stats[1] >= 1, stats
    W.check(small, names, num, use_excl=False, use_mask=False, use_fill=False)


def test_weight_one_and_no_arrays_are_the_rules_call(small):
    p = small.dp.p
    ones = W.DeviceWeighted(small.dp, W.Weighted(p, [np.full(cl.n_cols, W.ONE, np.uint32) for cl in p.clauses]), small.dr)
    for names in ((), ALL_RULES):
        want = small.dr.run(names, 20)
        for weights in ("own", [None] * len(p.clauses), [None, ones.dev[1], None]):
            got = ones.run(names, 20, weights=weights)
            W.compare(got, want)
            assert np.array_equal(got[3], want[3])


def test_idf_weights_from_the_device(gpu_session, small):
    p = small.dp.p
    dw = W.DeviceWeighted(small.dp, W.Weighted(p, device_idf(gpu_session, p, small.dp)), small.dr)
    plain = R.brute_force(p, 20, True, True, True, False)
    assert (W.brute_force(dw.wp, (), 20)[1] != plain[1]).any(), "idf changes some query's list"
    for num in (1, 20, 256):
        W.check(dw, (), num)
    W.check(dw, ALL_RULES, 20)


def test_idf_edge_cases(gpu_session):
    s = gpu_session
    for n_docs, df in ((100, [0, 1, 2, 3, 7, 50, 99, 100, 103]), (1, [0, 1, 4]), (10**15, [0, 1, 5, 10**6])):
        cp = np.concatenate([[0], np.cumsum(df)]).astype(np.int64)
        got = s.idf_weights(R._dev(s, cp), len(df), n_docs)
        s.synchronize()
        got = got.cpu().numpy().astype(np.int64)
        want = W.idf_ref(cp, n_docs).astype(np.int64)
        print("idf", n_docs, got.tolist(), want.tolist())
        assert np.abs(got - want).max() <= 1 and got[0] == 1 and got.min() >= 1 and got.max() <= W.MAX
    assert got[1] == W.MAX
    assert s.idf_weights(R._dev(s, cp), 0, 5).numel() == 0
    # 70 001 columns: more than one block, a last block that is not full; every df from 0 to beyond n_docs
    df = np.arange(70_001) % 5000
    cp = np.concatenate([[0], np.cumsum(df)]).astype(np.int64)
    got = s.idf_weights(R._dev(s, cp), df.size, 4000)
    s.synchronize()
    diff = np.abs(got.cpu().numpy().astype(np.int64) - W.idf_ref(cp, 4000).astype(np.int64))
    print("idf 70 001 columns: off by one unit at", int((diff == 1).sum()), "max", diff.max())
    assert diff.max() <= 1


def test_wide_catalogue_and_hub_columns(gpu_session):
    """70 000 items, three hub columns listed by 90 % of the item rows, half of the 64 queries hold them: the global class, tens of thousands of 64-bit
    counters raised and returned to zero per query, ids and backfill positions beyond 16 bits."""
    p = R.make_problem(22, 70_000, 64, cols=(70_000, 5000, 2000), boosts=(1.05, 20.0, 3.0), k=4, hist_hi=10, hub_cols=(5, 77, 40_000), hub_frac=0.9,
                       hub_query_frac=0.5)
    rules = RR.make_rules(p, 5)
    dp = R.DeviceProblem(gpu_session, p)
    w = W.random_weights(p, 42)
    w[0][[5, 77, 40_000]] = (W.MAX, 1, 12_345)
    dw = W.DeviceWeighted(dp, W.Weighted(p, w), RR.DeviceRules(dp, rules))
    for num in (1, 20, 256):
        stats = W.check(dw, (), num)
        assert 16 <= stats[1] <= 48 and stats[0] + stats[1] == 64
        W.check(dw, ("none", "range"), num)
    W.check(dw, (), 256, use_excl=False, use_mask=False, use_fill=False)
    W.check(dw, ALL_RULES, 20, no_backfill=True)
    W.check(dw, (), 20)      # once more: every fold returned its 64-bit counters to zero


@pytest.mark.parametrize("n_terms", [3072, 5000], ids=["lds_32bit", "global_64bit"])
def test_counter_bounds(gpu_session, n_terms):
    """One query of n_terms terms whose columns each hold the one item X, every weight the maximum.  3 072 terms: w(q) = 3 072, the LDS class, and its 32-bit
    counter ends at 3 072 * 2^20 > 2^31.  5 000 terms: the global class, and its counter ends at 5 000 * 2^20 > 2^32."""
    x = 4321
    p = W.one_item_problem(6000, n_terms, x, extra_queries=2)
    assert R.work_bound(p, True).tolist() == [n_terms, 1, 1] and _lib.REC_LDS_LIMIT == 3072
    wp = W.Weighted(p, [np.full(n_terms, W.MAX, np.uint32)])
    m = int(wp.m[0][0, x])
    assert m == n_terms << 20 and (m > 1 << 31 if n_terms == 3072 else m > 1 << 32) and wp.score[0, x] == n_terms * 32.0
    dw = W.DeviceWeighted(R.DeviceProblem(gpu_session, p), wp)
    for num in (1, 20):
        stats = W.check(dw, (), num)
        assert (int(stats[0]), int(stats[1])) == ((3, 0) if n_terms == 3072 else (2, 1))
    got = dw.run((), 1)
    assert got[1][0, 0] == x and got[2][0, 0] == n_terms * 32.0


def test_ties_between_different_term_sets_lds_class(gpu_session):
    """3 000 items, 1 800 listed, w = 2 700 and 2 950: the items at even positions reach M through one term, the others through two; the order at the
    num-th place follows the backfill position."""
    starts = (0, 250)
    p = W.tie_problem(25, 3000, 1800, starts)
    assert R.work_bound(p, True).tolist() == [2700, 2950]
    W.check_ties(gpu_session, p, starts, split=(2, 0))


def test_ties_between_different_term_sets_global_class(gpu_session):
    """70 000 items, all listed; the winners' positions start at 0, 250 and 65 530"""
    starts = (0, 250, 65_530)
    p = W.tie_problem(24, 70_000, 70_000, starts)
    assert R.work_bound(p, True).tolist() == [105_000, 105_250, 170_530]
    W.check_ties(gpu_session, p, starts, split=(0, 3))
