"""The cases of the hashed accumulator class (URCCO_REC_HASHED), shared by test_sim_recommend_hashed.py and test_gpu_recommend_hashed.py.  Every
case compares the flagged call (a) with the numpy restatement of the form in use (recommend_ref / _rules_ref / _weights_ref, imported as they are) and (b) with
the same call without the flag: counts, ids, score bits, stats[2] == 0, stats[3], stats[4], and the class split recommend_ref.work_bound predicts.  No tolerance."""
import functools
import itertools

import numpy as np
import torch

import recommend_ref as R
import recommend_rules_ref as RR
import recommend_weights_ref as W
from universal_recommender_amd import _lib

CAP, LIMIT, HASHED, AUTO = 1 << _lib.REC_HASH_CAP_LOG2, _lib.REC_HASH_LIMIT, _lib.REC_HASHED, _lib.REC_HASHED_AUTO
SMALL = (64, 256)   # URCCO_REC_LDS_LIMIT / URCCO_REC_HASH_LIMIT of the three-class problem
STARTS = (0, 1)
CASES = [("three", n) for n in (1, 20, 256)] + [("three_form", f) for f in ("rules", "idf")] + [("full", n, f) for n in (1, 20, 256) for f in (True, False)] + \
    [("wide",), ("auto_small",), ("auto_large",), ("python",)]


class Context:
    """the session, pytest's monkeypatch (the two limit knobs are read per call and undone after the test) and the problems already on the device"""

    def __init__(self, sess, monkeypatch):
        self.sess, self.env = sess, monkeypatch.setenv

    def dp(self, make):
        return device(self.sess, make)

    def limits(self, lds, hashed=LIMIT):
        self.env("URCCO_REC_LDS_LIMIT", str(lds))
        self.env("URCCO_REC_HASH_LIMIT", str(hashed))


@functools.lru_cache(None)
def device(sess, make):
    return R.DeviceProblem(sess, make())


def run(dp, num, flags, sw=(True, True, True, False), rules=None, weights=None):
    """sw: exclusions, mask, fill_order, NO_BACKFILL"""
    out = dp.sess.recommend(dp.n_queries, dp.p.n_items, dp.clauses, num, dp.excl if sw[0] else None, dp.mask if sw[1] else None, dp.fill if sw[2] else None,
                            flags | (_lib.REC_NO_BACKFILL if sw[3] else 0), rules=rules, weights=weights)
    dp.sess.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def check(ctx, dp, want, num, sw=(True, True, True, False), lims=(_lib.REC_LDS_LIMIT, LIMIT), **kw):
    """want: (count, idx, score, candidates, ...) of the restatement.  Returns the flagged call's statistics."""
    ctx.limits(*lims)
    got, plain = run(dp, num, HASHED, sw, **kw), run(dp, num, 0, sw, **kw)
    W.compare(got, want, f"restatement, num {num} switches {sw}")
    W.compare(got, plain, f"flagless call, num {num} switches {sw}")
    st, st0, w = got[3].tolist(), plain[3].tolist(), R.work_bound(dp.p, sw[0])
    lds, dense = int((w <= lims[0]).sum()), int((w > lims[1]).sum())
    print(f"num {num} switches {sw}: stats {st}, flagless {st0}, predicted LDS {lds}, dense {dense}")
    assert [st[0], st[5], st[1]] == [lds, dp.n_queries - lds - dense, dense] and [st0[0], st0[1], st0[5]] == [lds, dp.n_queries - lds, 0]
    assert st[2] == st0[2] == 0 and st[3] == st0[3] == want[3] and st[4] == st0[4] and st[6:] == [0, 0]
    return st


def three_problem():
    """300 items, 1 200 queries (every resident block serves several), a hub column: under SMALL all three classes serve"""
    return R.make_problem(11, 300, 1200, cols=(300, 500, 40), boosts=(1.05, 20.0, 0.3), k=6, hist_hi=12, hub_cols=(0,), hub_frac=1.0, hub_query_frac=0.2)


def three(ctx, num):
    dp = ctx.dp(three_problem)
    for sw in itertools.product((False, True), repeat=4):
        st = check(ctx, dp, R.brute_force(dp.p, num, *sw), num, sw, SMALL)
        assert min(st[0], st[5], st[1]) > 0


def three_form(ctx, form):
    """rules: ANY + NONE + RANGE, so that mask- and rule-rejected tombstones meet the backfill probe; idf: the weights read back from the device"""
    dp = ctx.dp(three_problem)
    if form == "rules":
        dr = RR.DeviceRules(dp, RR.make_rules(dp.p, 5))
        names = ("any", "none", "range")
        want = RR.brute_force(dp.p, [dr.rules[n] for n in names], 20)
        st = check(ctx, dp, want, 20, lims=SMALL, rules=[dr.dev[n] for n in names])
        assert st[4] == want[4] > 0
    else:
        w = [dp.sess.idf_weights(d[2], cl.n_cols, int(np.count_nonzero(np.diff(cl.ind_rp)))) for cl, d in zip(dp.p.clauses, dp.clauses)]
        dp.sess.synchronize()
        dw = W.DeviceWeighted(dp, W.Weighted(dp.p, [t.cpu().numpy().copy() for t in w]))
        st = check(ctx, dp, W.brute_force(dw.wp, (), 20), 20, lims=SMALL, weights=dw.dev)
    assert min(st[0], st[5], st[1]) > 0


def full_problem():
    """w = 98 304 (hashed: the limit itself, load factor 0.75) and 98 305 (dense) at the production limits; every candidate ties.  Two listed items have the
    last slot as their home by the published hash (the seed is chosen for that): the second of them wraps to the front of the table."""
    p = R.make_tie_problem(1, 400_000, LIMIT, STARTS)
    home = ((p.fill_order[:LIMIT].astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(32 - _lib.REC_HASH_CAP_LOG2)
    assert R.work_bound(p, True).tolist() == [LIMIT, LIMIT + 1] and int((home == CAP - 1).sum()) >= 2
    return p


def full(ctx, num, use_fill):
    dp = ctx.dp(full_problem)
    want = R.brute_force(dp.p, num, True, True, use_fill, False)
    assert not use_fill or all(np.array_equal(a, b) for a, b in zip(want[1:3], R.tie_rows(dp.p, STARTS, num)))
    st = check(ctx, dp, want, num, (True, True, use_fill, False))
    assert [st[0], st[5], st[1]] == [0, 1, 1]


def wide(ctx):
    """64-bit weighted counters: 4 100 columns list one item, the query holds them all at the maximum weight: M = 4 100 * 2^20 > 2^32, w = 4 100: hashed"""
    p = W.one_item_problem(50, 4100, 17, extra_queries=2)
    wp = W.Weighted(p, [np.full(4100, W.MAX, np.uint32)])
    dw = W.DeviceWeighted(R.DeviceProblem(ctx.sess, p), wp)
    want = W.brute_force(wp, (), 4)
    assert wp.m[0][0, 17] == 4100 << 20 > 1 << 32 and want[1][0, 0] == 17 and want[2][0, 0] == 1.0 * 4100 * 32.0
    assert check(ctx, dw.dp, want, 4, weights=dw.dev)[5] == 1


def blocks(sess, n_queries, bytes_per_block):
    """the documented block counts, from the session's CU count (the simulator's device has 8)"""
    n_cu = torch.cuda.get_device_properties(sess.device).multi_processor_count if sess.device.type == "cuda" else 8
    return max(1, min(2 * n_cu, n_queries, (512 << 20) // bytes_per_block))


def auto_small(ctx):
    """a small catalogue: the dense class has no fewer blocks than the hashed one, so AUTO leaves the call as it is"""
    dp = ctx.dp(three_problem)
    assert blocks(ctx.sess, dp.n_queries, 20 * dp.p.n_items) >= blocks(ctx.sess, dp.n_queries, CAP * 8 + LIMIT * 12)
    ctx.limits(*SMALL)
    got, plain = run(dp, 20, AUTO), run(dp, 20, 0)
    W.compare(got, R.brute_force(dp.p, 20, True, True, True, False), "AUTO, small catalogue (restatement)")
    W.compare(got, plain, "AUTO, small catalogue (flagless call)")
    assert np.array_equal(got[3], plain[3]) and got[3][5] == 0 and got[3][1] > 0


def auto_large(ctx, n_items=14_000_000, n_terms=4100, item=17):
    """14 M items, two tiny queries: one dense block (512 MiB / 20 B / 14 M = 1.9) against two hashed ones, so AUTO engages.  The restatement is written out --
    brute_force's dense n_queries x n_items matrices would take seconds here: the one listed item, then the backfill in item order (no mask, no fill_order)."""
    assert blocks(ctx.sess, 2, 20 * n_items) == 1 < blocks(ctx.sess, 2, CAP * 8 + LIMIT * 12) == 2
    irp = np.zeros(n_items + 1, np.int64)
    irp[item + 1:] = n_terms
    cl = R.Clause(n_terms, 1.5, irp, np.arange(n_terms, dtype=np.int32), np.array([0, n_terms, n_terms + 1]), np.append(np.arange(n_terms), 0).astype(np.int32))
    dp = R.DeviceProblem(ctx.sess, R.Problem(n_items, 2, [cl], np.zeros(3, np.int64), np.zeros(0, np.int32), np.ones(1, np.uint8), np.zeros(1, np.int32)))
    got, plain = (run(dp, 4, f, (False, False, False, False)) for f in (AUTO, 0))
    want = (np.full(2, 4, np.int32), np.tile(np.array([item, 0, 1, 2], np.int32), (2, 1)), np.array([[1.5 * n_terms, 0, 0, 0], [1.5, 0, 0, 0]]))
    W.compare(got, want, "AUTO, large catalogue (restatement)")
    W.compare(got, plain, "AUTO, large catalogue (flagless call)")
    assert got[3].tolist() == [1, 0, 0, 2, 0, 1, 0, 0] and plain[3].tolist() == [1, 1, 0, 2, 0, 0, 0, 0]


def python(ctx):
    """the handmade golden model: accumulator="hashed" gives the default results; with the LDS class closed (limit 0) every query with a term is hashed"""
    from test_explain_predict import QUERIES
    from test_recommend_rules_golden import NOW_MS, _stack
    from universal_recommender_amd.history import DeviceHistory
    algo, model, _, history, *_ = _stack(ctx.sess)
    dh, users = DeviceHistory.from_dict(ctx.sess, model, history), list(history) + ["nobody"]
    want = algo.batch_predict(model, QUERIES, dh, now_ms=NOW_MS)
    rows = algo.user_recommendations(model, dh, users, num=6, now_ms=NOW_MS, explain=3)
    ctx.limits(0)
    assert algo.batch_predict(model, QUERIES, dh, now_ms=NOW_MS, accumulator="hashed") == want
    got = algo.user_recommendations(model, dh, users, num=6, now_ms=NOW_MS, explain=3, accumulator="hashed")
    assert got[7] == rows[7] and all(torch.equal(a, b) for a, b in zip(got[:7], rows[:7]))
