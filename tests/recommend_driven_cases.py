"""The cases of the driven class (URCCO_REC_DRIVEN), shared by test_sim_recommend_driven.py and test_gpu_recommend_driven.py.  Every case compares
the flagged call (a) with the numpy restatement as it stands (recommend_rules_ref / recommend_weights_ref) and (b) with the same call without the flag: counts,
ids and score bits (no tolerance), stats[2] == 0, stats[3], and the class split, gathered items and walk steps predicted on the host from d(q)."""
import functools
import itertools

import numpy as np
import pytest

import recommend_hashed_cases as H
import recommend_ref as R
import recommend_rules_ref as RR
import recommend_weights_ref as W
from universal_recommender_amd import _lib

DRIVEN, LIMIT, TERMS = _lib.REC_DRIVEN, _lib.REC_DRIVE_LIMIT, 4096   # TERMS: REC_DRV_TERMS of csrc/cco_recommend.h, the staged query-term entries
SMALL = 64   # URCCO_REC_DRIVE_LIMIT of the 300-item problem
ON = (True, True, True, False)
CASES = [("mixed", n) for n in (1, 20, 256)] + [("mixed", 20, True)] + [("edge", n, f) for n in (1, 256) for f in (True, False)] + \
    [("two_drivers",), ("weighted",), ("wide",), ("long_terms",), ("python",)]


def csc(sess, r):
    """the CSC of an ANY rule's matrix (entries outside 0..n_cols cannot be listed; a duplicated entry is listed twice), on the device"""
    rows = np.repeat(np.arange(r.m_rp.size - 1, dtype=np.int32), np.diff(r.m_rp))
    keep = (r.m_ci >= 0) & (r.m_ci < r.n_cols)
    order = np.argsort(r.m_ci[keep], kind="stable")
    cp = np.zeros(r.n_cols + 1, np.int64)
    np.cumsum(np.bincount(r.m_ci[keep], minlength=r.n_cols), out=cp[1:])
    return R._dev(sess, cp), R._dev(sess, rows[keep][order])


def bound(p, r):
    """d_r(q): the summed lengths of the columns the query's rule row names"""
    col_len = np.bincount(r.m_ci[(r.m_ci >= 0) & (r.m_ci < r.n_cols)], minlength=r.n_cols)
    q = np.repeat(np.arange(p.n_queries), np.diff(r.q_rp))
    ok = (r.q_ci >= 0) & (r.q_ci < r.n_cols)
    return np.bincount(q[ok], weights=col_len[r.q_ci[ok]], minlength=p.n_queries).astype(np.int64)


def walk_steps(p, score, ok, num, sw):
    """recommend_rules_ref.brute_force's backfill steps, per query"""
    positive, zero = ok & (score > 0), ok & ~(score > 0)
    need = num - np.minimum(positive.sum(1), num)
    reached = np.cumsum(zero[:, p.fill_order] if sw[2] else zero, 1) >= need[:, None]
    per_query = np.where(reached.any(1), reached.argmax(1) // RR.STEP + 1, -(-p.n_items // RR.STEP))
    return np.where((need > 0) & (not sw[3]), per_query, 0)


def plan(p, rules, drive, limit):
    """(d(q), index into `drive` of the driving rule, driven?) -- the lowest rule index wins a tie"""
    d = np.stack([bound(p, rules[j]) for j in drive])
    return d.min(0), d.argmin(0), d.min(0) <= limit


def check(ctx, dp, dev_rules, rules, drive, want, score, num, sw=ON, lims=(LIMIT, _lib.REC_LDS_LIMIT, H.LIMIT), flags=0, weights=None):
    """rules: the Rule objects in call order; drive: indices of the drivers among them.  Returns the flagged call's statistics."""
    ctx.env("URCCO_REC_DRIVE_LIMIT", str(lims[0]))
    ctx.limits(*lims[1:])
    args = (dp.n_queries, dp.p.n_items, dp.clauses, num, dp.excl if sw[0] else None, dp.mask if sw[1] else None, dp.fill if sw[2] else None)
    kw = dict(rules=dev_rules, weights=weights)
    drivers = [(j, *csc(dp.sess, rules[j])) for j in drive]
    rows = [(R._dev(dp.sess, cl.ind_rp), R._dev(dp.sess, cl.ind_ci.astype(np.int32))) for cl in dp.p.clauses]
    nb = _lib.REC_NO_BACKFILL if sw[3] else 0
    got = dp.sess.recommend(*args, flags | nb | DRIVEN, drivers=drivers, clause_rows=rows, **kw)
    plain = dp.sess.recommend(*args, flags | nb, **kw)
    dp.sess.synchronize()
    got, plain = (tuple(t.cpu().numpy() for t in out) for out in (got, plain))
    W.compare(got, want, f"restatement, num {num} switches {sw}")
    W.compare(got, plain, f"flagless call, num {num} switches {sw}")
    _, who, driven = plan(dp.p, rules, drive, lims[0])
    steps = walk_steps(dp.p, score, RR.brute_force(dp.p, rules, num, *sw)[6], num, sw)   # [6]: the eligibility, which no weight changes
    gathered = sum(int(rules[drive[j]].ok[q].sum()) for q, j in zip(np.nonzero(driven)[0], who[driven]))   # an ANY rule's ok row IS E_r(q)
    st, st0 = got[3].tolist(), plain[3].tolist()
    print(f"num {num} switches {sw}: stats {st}, flagless {st0}, predicted driven {int(driven.sum())}, gathered {gathered}")
    assert st[6] == int(driven.sum()) and st[0] + st[1] + st[5] + st[6] == dp.n_queries and st[7] == gathered and st0[6:] == [0, 0]
    assert st[2] == st0[2] == 0 and st[3] == st0[3] == want[3]
    assert st[4] == int(steps[~driven].sum()) and st0[4] == int(steps.sum()) == want[4]
    return st


@functools.lru_cache(None)
def mixed_setup(sess):
    """the three-class problem of the hashed cases under "any" + "none" + "range", and what it must hold, asserted on the restatement alone (num 20)"""
    dp = H.device(sess, H.three_problem)
    p, dr = dp.p, RR.DeviceRules(dp, RR.make_rules(dp.p, 5))
    rules = [dr.rules[n] for n in ("any", "none", "range")]
    count, _, sc, *_ = RR.brute_force(p, rules, 20)
    d, _, driven = plan(p, rules, [0], SMALL)
    listed = rules[0].ok
    struck = np.zeros_like(listed)
    struck[np.repeat(np.arange(p.n_queries), np.diff(p.excl_rp)), p.excl_ci] = True
    assert driven.any() and not driven.all(), "driven and not-driven are both populated"
    assert (d[driven] == 3).any() and (d[driven] == 0).any(), "the rare value and the empty rows are driven"
    assert (d > listed.sum(1))[driven].any(), "a driven query with an item that holds two of its values"
    assert (listed & struck).any(1)[driven].any(), "a driven query with an exclusion that strikes a listed item"
    assert ((count > 0) & (count < 20))[driven].any(), "a driven query with 0 < count < num"
    last = sc[np.arange(p.n_queries), np.maximum(count, 1) - 1]
    assert ((count > 1) & (sc[:, 0] > 0) & (last == 0))[driven].any(), "a driven query with a positive winner followed by zero-score ones"
    return dp, dr, rules


def mixed(ctx, num, four=False):
    """four: LDS limit 64, hash limit 256, drive limit 64 under URCCO_REC_HASHED, so that all four classes serve in one call"""
    dp, dr, rules = mixed_setup(ctx.sess)
    dev = [dr.dev[n] for n in ("any", "none", "range")]
    for sw in [ON] if four else itertools.product((False, True), repeat=4):
        want, lims = RR.brute_force(dp.p, rules, num, *sw), (SMALL,) + (H.SMALL if four else (_lib.REC_LDS_LIMIT, H.LIMIT))
        st = check(ctx, dp, dev, rules, [0], want, dp.p.cache[(None, None, sw[2])][0], num, sw, lims, H.HASHED if four else 0)
        assert not four or min(st[0], st[5], st[1], st[6]) > 0


@functools.lru_cache(None)
def edge_setup(sess, n=8192):
    """the production limit: value 0 is held by exactly 3072 items (driven, load factor 0.75 exactly), value 1 by 3073 (walk); five items score, the rest tie at 0"""
    rng = np.random.default_rng(3)
    a, b = rng.permutation(n)[:LIMIT], rng.permutation(n)[:LIMIT + 1]
    in_a, in_b = np.isin(np.arange(n), a), np.isin(np.arange(n), b)
    held = [np.nonzero([in_a[i], in_b[i]])[0] for i in range(n)]
    hot = np.intersect1d(a, b)[:5]
    irp = np.zeros(n + 1, np.int64)
    np.cumsum(np.isin(np.arange(n), hot), out=irp[1:])
    cl = R.Clause(1, 1.5, irp, np.zeros(hot.size, np.int32), np.arange(3, dtype=np.int64), np.zeros(2, np.int32))
    excl = [np.array([hot[0], a[7]]), np.array([hot[1]])]
    p = R.Problem(n, 2, [cl], *R._rows_to_csr(excl), (rng.random(n) >= 0.1).astype(np.uint8), rng.permutation(n).astype(np.int32))
    R.dense_matches(p)
    rule = RR.Rule(_lib.RULE_ANY, 2, *R._rows_to_csr(held, np.int64), np.arange(3, dtype=np.int64), np.arange(2, dtype=np.int64))
    rule.ok = RR._eligibility(p, rule)
    assert bound(p, rule).tolist() == [LIMIT, LIMIT + 1] and hot.size == 5
    dp = R.DeviceProblem(sess, p)
    return dp, RR.DeviceRules(dp, {"any": rule}), [rule]


def edge(ctx, num, use_fill):
    dp, dr, rules = edge_setup(ctx.sess)
    sw = (True, True, use_fill, False)
    st = check(ctx, dp, [dr.dev["any"]], rules, [0], RR.brute_force(dp.p, rules, num, *sw), dp.p.cache[(None, None, use_fill)][0], num, sw)
    assert st[6] == 1 and st[7] == LIMIT


def two_drivers(ctx):
    """"any" and "ind" (clause 1's indicator matrix as an ANY rule) both drive: the smaller bound per query; the results are those of either one alone"""
    dp, dr, _ = mixed_setup(ctx.sess)
    rules, dev = [dr.rules[n] for n in ("any", "ind")], [dr.dev[n] for n in ("any", "ind")]
    _, who, driven = plan(dp.p, rules, [0, 1], SMALL)
    assert (who[driven] == 0).any() and (who[driven] == 1).any(), "each of the two drives some query"
    want, score = RR.brute_force(dp.p, rules, 20), dp.p.cache[(None, None, True)][0]
    for drive in ([0, 1], [0], [1]):
        check(ctx, dp, dev, rules, drive, want, score, 20, ON, (SMALL, _lib.REC_LDS_LIMIT, H.LIMIT))


def weighted(ctx):
    """`mixed` at num 20 under the idf weights read back from the device"""
    dp, dr, rules = mixed_setup(ctx.sess)
    w = [dp.sess.idf_weights(d[2], cl.n_cols, int(np.count_nonzero(np.diff(cl.ind_rp)))) for cl, d in zip(dp.p.clauses, dp.clauses)]
    dp.sess.synchronize()
    dw = W.DeviceWeighted(dp, W.Weighted(dp.p, [t.cpu().numpy().copy() for t in w]))
    check(ctx, dp, [dr.dev[n] for n in ("any", "none", "range")], rules, [0], W.brute_force(dw.wp, rules, 20), dw.wp.score, 20, ON,
          (SMALL, _lib.REC_LDS_LIMIT, H.LIMIT), weights=dw.dev)


def wide(ctx):
    """64-bit sums in one candidate: 4 100 columns list item 17, the query holds them all at the maximum weight, and item 17 alone holds the rule's value"""
    p = W.one_item_problem(50, 4100, 17, extra_queries=2)
    wp = W.Weighted(p, [np.full(4100, W.MAX, np.uint32)])
    held = [np.zeros(int(i == 17), np.int64) for i in range(50)]
    rule = RR.Rule(_lib.RULE_ANY, 1, *R._rows_to_csr(held, np.int64), np.arange(4, dtype=np.int64), np.zeros(3, np.int64))
    rule.ok = RR._eligibility(p, rule)
    dw = W.DeviceWeighted(R.DeviceProblem(ctx.sess, p), wp, RR.DeviceRules(R.DeviceProblem(ctx.sess, p), {"any": rule}))
    want = W.brute_force(wp, [rule], 4)
    assert wp.m[0][0, 17] == 4100 << 20 > 1 << 32 and want[0].tolist() == [1, 1, 1] and want[1][0, 0] == 17 and want[2][0, 0] == 4100 * 32.0
    assert check(ctx, dw.dp, [dw.dr.dev["any"]], [rule], [0], want, wp.score, 4, weights=dw.dev)[6] == 3


def long_terms(ctx, n=64, n_cols=4200):
    """the staging capacity: query 0's term row holds TERMS entries (searched in LDS), query 1's one more (searched in global memory); both rows end inside the
    columns the item rows list, so the last staged entry and the first one beyond it are both matched"""
    rng = np.random.default_rng(9)
    ind = [np.unique(np.concatenate([rng.integers(0, n_cols, 4), rng.integers(TERMS - 4, TERMS + 3, 3)])) for _ in range(n)]
    cl = R.Clause(n_cols, 1.25, *R._rows_to_csr(ind), *R._rows_to_csr([np.arange(TERMS), np.arange(TERMS + 1)]))
    p = R.Problem(n, 2, [cl], np.zeros(3, np.int64), np.zeros(0, np.int32), np.ones(n, np.uint8), rng.permutation(n).astype(np.int32))
    R.dense_matches(p)
    held = [np.zeros(int(i % 3 == 0), np.int64) for i in range(n)]
    rule = RR.Rule(_lib.RULE_ANY, 1, *R._rows_to_csr(held, np.int64), np.arange(3, dtype=np.int64), np.zeros(2, np.int64))
    rule.ok = RR._eligibility(p, rule)
    assert any(TERMS - 1 in r for r in ind[::3]) and any(TERMS in r for r in ind[::3]) and np.diff(cl.q_rp).tolist() == [TERMS, TERMS + 1]
    dp = R.DeviceProblem(ctx.sess, p)
    want = RR.brute_force(p, [rule], 20)
    assert not np.array_equal(want[2][0], want[2][1])
    assert check(ctx, dp, [RR.DeviceRules(dp, {"any": rule}).dev["any"]], [rule], [0], want, p.cache[(None, None, True)][0], 20)[6] == 2


def python(ctx):
    """the handmade golden model: filter_plan="driven" gives the default results -- the explain queries plus a category that holds fewer items than num and a
    category combined with a dateRange and the user's history as a filter"""
    import torch
    from test_explain_predict import QUERIES
    from test_recommend_rules_golden import NOW_MS, _stack
    from universal_recommender_amd.history import DeviceHistory
    algo, model, _, history, *_ = _stack(ctx.sess)
    dh, users = DeviceHistory.from_dict(ctx.sess, model, history), list(history) + ["nobody"]
    cats = model.properties["categories"]
    held = dict(zip(cats.values, np.diff(cats.col_ptr.cpu().numpy()[:cats.n_cols + 1]).tolist()))
    rare = min(held, key=lambda v: (held[v], v))
    queries = list(QUERIES) + [
        {"user": users[0], "num": 20, "fields": [{"name": "categories", "values": [rare], "bias": -1}]},
        {"user": users[1], "num": 4, "userBias": -1, "fields": [{"name": "categories", "values": sorted(held)[:2], "bias": -1}],
         "dateRange": {"name": "date", "after": "2000-01-01T00:00:00.000Z"}}]
    want = algo.batch_predict(model, queries, dh, now_ms=NOW_MS)
    assert 0 < held[rare] < 20 and len(want[-2]["itemScores"]) <= held[rare], "the rare category holds fewer items than num"
    assert algo.batch_predict(model, queries, dh, now_ms=NOW_MS, filter_plan="driven") == want
    with pytest.raises(ValueError):
        algo.predict(model, queries[0], dh, now_ms=NOW_MS, filter_plan="list")
    rows = algo.user_recommendations(model, dh, users, num=6, now_ms=NOW_MS, explain=3)
    got = algo.user_recommendations(model, dh, users, num=6, now_ms=NOW_MS, explain=3, filter_plan="driven")
    assert got[7] == rows[7] and all(torch.equal(a, b) for a, b in zip(got[:7], rows[:7]))
