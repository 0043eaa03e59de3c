"""urcco_dev_recommend_weighted and urcco_dev_idf_weights on the host simulator (kernel LOGIC on the CPU) against the restatement of decision D20
(tests/recommend_weights_ref.py): counts, ids, score bits and stats[0..4] exact.  The 300-item x 200-query problem of test_sim_recommend.py with
URCCO_REC_LDS_LIMIT lowered to 256, so that both classes -- the 32-bit LDS counters and the 64-bit global ones -- serve queries in every run."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recommend_ref as R
import recommend_rules_ref as RR
import recommend_weights_ref as W
from universal_recommender_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_LIMIT = 256
ALL_RULES = ("any", "none", "range", "ind")


@pytest.fixture(scope="module")
def problem():
    p = R.make_problem(11, 300, 200, cols=(300, 500, 7), boosts=(1.05, 20.0, 0.3), k=10, hist_hi=30, hub_cols=(0,), hub_frac=1.0, hub_query_frac=0.25)
    return p, RR.make_rules(p, 5)


@pytest.fixture(scope="module")
def base(sim_session, problem):
    dp = R.DeviceProblem(sim_session, problem[0])
    return dp, RR.DeviceRules(dp, problem[1])


@pytest.fixture(scope="module")
def dev(base, problem):
    """random weights on clauses 0 and 2, clause 1 without an array"""
    w = W.random_weights(problem[0], 31, without=(1,))
    assert w[1] is None and W.extremes_hit(problem[0], w)
    return W.DeviceWeighted(base[0], W.Weighted(problem[0], w), base[1])


@pytest.fixture()
def low_limit():
    os.environ["URCCO_REC_LDS_LIMIT"] = str(SIM_LIMIT)
    yield SIM_LIMIT
    del os.environ["URCCO_REC_LDS_LIMIT"]


@pytest.mark.parametrize("num", [1, 4, 20])
def test_every_combination_matches_the_restatement(dev, num, low_limit):
    for use_excl, use_mask, use_fill, no_backfill in itertools.product((False, True), repeat=4):
        stats = W.check(dev, (), num, use_excl, use_mask, use_fill, no_backfill, lds_limit=low_limit)
        assert stats[0] > 0 and stats[1] > 0, stats


@pytest.mark.parametrize("num", [1, 20])
def test_every_combination_under_rules(dev, num, low_limit):
    for use_excl, use_mask, use_fill, no_backfill in itertools.product((False, True), repeat=4):
        stats = W.check(dev, ALL_RULES, num, use_excl, use_mask, use_fill, no_backfill, lds_limit=low_limit)
        assert stats[0] > 0 and stats[1] > 0 and (stats[4] == 0) == no_backfill, stats


def test_production_limit_and_every_clause_weighted(base, problem):
    w = W.random_weights(problem[0], 32)
    dw = W.DeviceWeighted(base[0], W.Weighted(problem[0], w), base[1])
    stats = W.check(dw, (), 20)
    assert stats[0] == dw.dp.n_queries and stats[1] == 0
    W.check(dw, ("any", "range"), 4)


def test_the_weights_change_the_order(dev):
    """the problem is no trivial one: some query's top 20 differs from the unweighted call's"""
    plain = R.brute_force(dev.dp.p, 20, True, True, True, False)
    weighted = W.brute_force(dev.wp, (), 20)
    assert np.array_equal(plain[0], weighted[0]) and (plain[1] != weighted[1]).any()


@pytest.mark.parametrize("names", [(), ALL_RULES], ids=["plain", "rules"])
def test_weight_one_and_no_arrays_are_the_rules_call_bit_for_bit(base, problem, names, low_limit):
    p = problem[0]
    ones = [np.full(cl.n_cols, W.ONE, np.uint32) for cl in p.clauses]
    dw = W.DeviceWeighted(base[0], W.Weighted(p, ones), base[1])
    for num, no_backfill in ((1, False), (20, False), (20, True)):
        rules = base[1].run(names, num, no_backfill=no_backfill)                    # urcco_dev_recommend_rules
        for weights in ("own", [None] * len(p.clauses), [dw.dev[0], None, None]):
            got = dw.run(names, num, no_backfill=no_backfill, weights=weights)
            W.compare(got, rules, f"weights {weights if weights == 'own' else [w is not None for w in weights]}")
            assert np.array_equal(got[3], rules[3])
        W.check(dw, names, num, no_backfill=no_backfill, lds_limit=low_limit)
    # the array itself NULL, through the raw symbol
    s, dp, nq, num = base[0].sess, base[0], p.n_queries, 4
    arr = (_lib.RecClause * len(dp.clauses))()
    for c, (n_cols, boost, cp, ri, qrp, qci) in enumerate(dp.clauses):
        arr[c].n_cols, arr[c].boost = n_cols, boost
        arr[c].ind_col_ptr, arr[c].ind_row_idx, arr[c].q_row_ptr, arr[c].q_col_idx = cp.data_ptr(), ri.data_ptr(), qrp.data_ptr(), qci.data_ptr()
    cnt, idx, sc, st = s.empty(nq, torch.int32), s.empty(nq * num, torch.int32), s.empty(nq * num, torch.float64), s.empty(_lib.REC_STATS_LEN, torch.int64)
    assert s.lib.urcco_dev_recommend_weighted(s.handle, nq, p.n_items, arr, len(dp.clauses), None, None, None, None, num, 0, cnt.data_ptr(), idx.data_ptr(),
                                              sc.data_ptr(), st.data_ptr(), None, 0, None) == _lib.OK
    s.synchronize()
    want = dp.run(num, use_excl=False, use_mask=False, use_fill=False)
    W.compare((cnt.numpy(), idx.numpy().reshape(nq, num), sc.numpy().reshape(nq, num)), want, "clause_weights == NULL")
    assert np.array_equal(st.numpy(), want[3])


def test_a_weight_of_zero_counts_as_one_and_one_above_the_maximum_as_the_maximum(base, problem, low_limit):
    p = problem[0]
    good = W.random_weights(p, 33)
    bad = [w.copy() for w in good]
    for g, b in zip(good, bad):
        b[g == 1] = 0
        b[g == W.MAX] = np.array([W.MAX + 1, 0xffffffff] * g.size, np.uint32)[: int((g == W.MAX).sum())]
        b[-1], g[-1] = 0xffffffff, W.MAX
        b[-2], g[-2] = 0, 1
    assert any((b == 0).any() for b in bad) and any((b > W.MAX).any() for b in bad)
    dg = W.DeviceWeighted(base[0], W.Weighted(p, good))
    db = W.DeviceWeighted(base[0], W.Weighted(p, bad))
    assert np.array_equal(dg.wp.score.view(np.int64), db.wp.score.view(np.int64))     # the restatement clamps too
    for num in (4, 20):
        a, b = dg.run((), num), db.run((), num)
        W.compare(b, a, "clamped")
        assert np.array_equal(a[3], b[3]) and a[3][0] > 0 and a[3][1] > 0
        W.check(db, (), num, lds_limit=low_limit)


@pytest.mark.parametrize("n_terms,limit", [(40, 64), (90, 64)], ids=["lds", "global"])
def test_counter_bounds_small(sim_session, n_terms, limit):
    """the construction of the GPU file's counter tests at simulator size: every term lists the one item and weighs the maximum"""
    os.environ["URCCO_REC_LDS_LIMIT"] = str(limit)
    try:
        p = W.one_item_problem(50, n_terms, 17, extra_queries=2)
        wp = W.Weighted(p, [np.full(n_terms, W.MAX, np.uint32)])
        assert wp.m[0][0, 17] == n_terms << 20 and wp.score[0, 17] == n_terms * 32.0
        stats = W.check(W.DeviceWeighted(R.DeviceProblem(sim_session, p), wp), (), 4, lds_limit=limit)
        assert int(stats[1]) == (1 if n_terms > limit else 0)
    finally:
        del os.environ["URCCO_REC_LDS_LIMIT"]


TIE_STARTS = (0, 250)


@pytest.mark.parametrize("limit", [_lib.REC_LDS_LIMIT, SIM_LIMIT], ids=["lds", "global"])
def test_ties_between_different_term_sets(sim_session, limit):
    """Three columns instead of make_tie_problem's one; the items listing column 0 (weight 3 * ONE / 2) and those listing columns 1 and 2 (ONE / 2 + ONE) sum
    to the same M: the cut inside the tie follows the backfill position.  w(q) = 2 700 and 2 950: the LDS class under the production limit."""
    p = W.tie_problem(25, 3000, 1800, TIE_STARTS)
    assert R.work_bound(p, True).tolist() == [2700, 2950]
    os.environ["URCCO_REC_LDS_LIMIT"] = str(limit)
    try:
        W.check_ties(sim_session, p, TIE_STARTS, (2, 0) if limit == _lib.REC_LDS_LIMIT else (0, 2), lds_limit=limit)
    finally:
        del os.environ["URCCO_REC_LDS_LIMIT"]


IDF_DF = [0, 1, 2, 3, 7, 50, 99, 100, 103]     # n_docs = 100: df in {0, 1, n_docs, n_docs + 3} and a few between


def idf_col_ptr(df):
    return np.concatenate([[0], np.cumsum(df)]).astype(np.int64)


@pytest.mark.parametrize("n_docs", [100, 1, 10**15])
def test_idf_weights_are_within_one_unit_of_numpy(sim_session, n_docs):
    s = sim_session
    df = IDF_DF if n_docs != 1 else [0, 1, 4]
    cp = idf_col_ptr(df)
    got = s.idf_weights(R._dev(s, cp), len(df), n_docs)
    s.synchronize()
    got = got.cpu().numpy().astype(np.int64)
    want = W.idf_ref(cp, n_docs).astype(np.int64)
    print("idf", n_docs, got.tolist(), want.tolist())
    assert np.abs(got - want).max() <= 1 and got.min() >= 1 and got.max() <= W.MAX
    assert got[0] == 1, "a column nothing lists"
    if n_docs == 100:
        assert got[-1] == got[-2], "df > n_docs counts as n_docs"
        assert (np.diff(got[1:-1]) < 0).all(), "rarer terms weigh more"
    if n_docs == 10**15:
        assert got[1] == W.MAX, "clamped to the maximum"


def test_idf_weights_no_columns_and_bad_arguments(sim_session):
    s = sim_session
    cp = R._dev(s, idf_col_ptr([1, 2]))
    assert s.idf_weights(cp, 0, 5).numel() == 0
    out = s.empty(2, torch.uint32)
    assert s.lib.urcco_dev_idf_weights(s.handle, 0, None, 1, None) == _lib.OK
    for n_cols, col_ptr, n_docs, o in ((-1, cp, 5, out), (2, cp, 0, out), (2, cp, -3, out), (2, None, 5, out), (2, cp, 5, None)):
        assert s.lib.urcco_dev_idf_weights(s.handle, n_cols, col_ptr.data_ptr() if col_ptr is not None else None, n_docs,
                                           o.data_ptr() if o is not None else None) == _lib.BAD_ARG
    assert s.lib.urcco_dev_idf_weights(None, 2, cp.data_ptr(), 5, out.data_ptr()) == _lib.BAD_ARG


def test_scores_with_device_idf_weights(base, problem, low_limit):
    """the weights read back from the device feed the restatement: exact"""
    p, (dp, dr) = problem[0], base
    w = []
    for cl, dcl in zip(p.clauses, dp.clauses):
        n_docs = int(np.count_nonzero(np.diff(cl.ind_rp)))
        t = dp.sess.idf_weights(dcl[2], cl.n_cols, n_docs)
        dp.sess.synchronize()
        w.append(t.cpu().numpy().copy())
        cp = np.concatenate([[0], np.cumsum(np.bincount(cl.ind_ci, minlength=cl.n_cols))])
        assert np.abs(w[-1].astype(np.int64) - W.idf_ref(cp, n_docs).astype(np.int64)).max() <= 1
    dw = W.DeviceWeighted(dp, W.Weighted(p, w), dr)
    W.check(dw, (), 20, lds_limit=low_limit)
    W.check(dw, ALL_RULES, 4, lds_limit=low_limit)


def test_bad_arguments(dev):
    s, dp = dev.dp.sess, dev.dp

    def status(**kw):
        args = dict(n_queries=dp.n_queries, n_items=dp.p.n_items, clauses=dp.clauses, num=4, weights=dev.dev)
        args.update(kw)
        with pytest.raises(_lib.UrccoError) as ei:
            s.recommend(**args)
        return ei.value.status

    assert status(num=0) == _lib.BAD_ARG and status(num=257) == _lib.BAD_ARG
    assert status(clauses=[dp.clauses[c % 3] for c in range(17)], weights=[None] * 17) == _lib.BAD_ARG
    assert status(clauses=[(dp.clauses[0][0], float("nan")) + tuple(dp.clauses[0][2:])], weights=[dev.dev[0]]) == _lib.BAD_ARG
    assert status(flags=2) == _lib.BAD_ARG
    assert status(rules=[dev.dr.dev["any"]] * 17) == _lib.BAD_ARG
    assert status(rules=[(3,) + dev.dr.dev["any"][1:]]) == _lib.BAD_ARG
    assert status(rules=[dev.dr.dev["range"][:3] + (None,)]) == _lib.BAD_ARG
    with pytest.raises(ValueError):
        s.recommend(dp.n_queries, dp.p.n_items, dp.clauses, 4, weights=dev.dev[:2])
    with pytest.raises(ValueError):
        s.recommend(dp.n_queries, dp.p.n_items, dp.clauses, 4, weights=[dev.dev[0].view(torch.int32), None, None])
    # through the raw symbol: a half-NULL exclusion pair, rules == NULL with n_rules > 0, no session
    nq, num = dp.n_queries, 4
    cnt, idx, sc = torch.zeros(nq, dtype=torch.int32), torch.zeros(nq * num, dtype=torch.int32), torch.zeros(nq * num, dtype=torch.float64)
    arr = (_lib.RecClause * 1)()
    wp = (_lib.C.c_void_p * 1)()
    f = s.lib.urcco_dev_recommend_weighted
    assert f(s.handle, nq, dp.p.n_items, arr, 0, dp.excl[0].data_ptr(), None, None, None, num, 0, cnt.data_ptr(), idx.data_ptr(), sc.data_ptr(), None, None, 0, wp) == _lib.BAD_ARG
    assert f(s.handle, nq, dp.p.n_items, arr, 0, None, None, None, None, num, 0, cnt.data_ptr(), idx.data_ptr(), sc.data_ptr(), None, None, 1, wp) == _lib.BAD_ARG
    assert f(None, nq, dp.p.n_items, arr, 0, None, None, None, None, num, 0, cnt.data_ptr(), idx.data_ptr(), sc.data_ptr(), None, None, 0, wp) == _lib.BAD_ARG


def test_under_guard_pages():
    """This module once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument): a weight read past its
    array, or a 64-bit counter past its slice, would fault."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    env = dict(os.environ, HIPSIM_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
