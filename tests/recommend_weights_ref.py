"""Shared by the term-weight tests: tests/recommend_ref.py's and tests/recommend_rules_ref.py's seeded problems (imported unchanged) with per-clause weight
arrays, and the brute-force restatement of DESIGN.md decision D20.

The restatement, word for word: per clause the dense integer matrix M_c = T_c diag(w_c) I_c' of the 0/1 matrices and the integer weights (int64: the
largest sum of the tests, 5 000 * 2^20, is far below 2^63), a clause without an array counting URCCO_REC_WEIGHT_ONE per term and a stored weight clamped
into 1 .. URCCO_REC_WEIGHT_MAX; score = ((0.0 + boost_0 * (float64(M_0) * 2^-15)) + boost_1 * (float64(M_1) * 2^-15)) + ... in a Python loop over the
clauses (float64, one rounding per operation); eligibility (exclusion row, item mask, the rules' dense matrices of recommend_rules_ref); np.lexsort on
(backfill position, -score); the cut to num.  Counts, ids, score bits and stats[0..4] are compared for exact equality: the M_c are integers and the sum
has a fixed order, so there is no tolerance to choose.

idf_ref restates urcco_dev_idf_weights in numpy.  The device's f64 log and numpy's may differ by a few ulp, which is far below 2^-15, so the two integers can
differ only where idf * 2^15 sits next to a rounding tie: by one unit at the most -- the bound the tests assert.  The score tests use the weights read back
from the device, so they stay exact."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import scipy.sparse as sp

import recommend_ref as R
import recommend_rules_ref as RR
from universal_recommender_amd import _lib

ONE, MAX = _lib.REC_WEIGHT_ONE, _lib.REC_WEIGHT_MAX
UNIT = np.float64(2.0 ** -15)
STEP = RR.STEP


def idf_ref(col_ptr: np.ndarray, n_docs: int) -> np.ndarray:
    """clamp(rint(log(1 + (n_docs - df + 0.5) / (df + 0.5)) * 2^15), 1, MAX) with df = the column length clamped to n_docs; df == 0 gives 1 (np.rint and
    llrint both round ties to even)."""
    df = np.minimum(np.diff(np.asarray(col_ptr, np.int64)), n_docs)
    idf = np.log(np.float64(1.0) + ((n_docs - df).astype(np.float64) + 0.5) / (df.astype(np.float64) + 0.5))
    w = np.clip(np.rint(idf * np.float64(ONE)), 1, MAX)
    w[df <= 0] = 1
    return w.astype(np.uint32)


def random_weights(p: R.Problem, seed: int, without: Sequence[int] = ()) -> List[Optional[np.ndarray]]:
    """One uint32 array per clause (None for the clauses in `without`): log-uniform in 1 .. MAX so that small and large weights both occur, both extremes
    placed on columns that queries hold and items list (asserted by the callers through `extremes_hit`)."""
    rng = np.random.default_rng(seed)
    out: List[Optional[np.ndarray]] = []
    for c, cl in enumerate(p.clauses):
        if c in without:
            out.append(None)
            continue
        w = np.exp2(rng.random(cl.n_cols) * 20.0).astype(np.uint32)
        w = np.clip(w, 1, MAX)
        used = np.intersect1d(cl.q_ci, cl.ind_ci)
        if used.size >= 2:
            w[used[0]], w[used[-1]] = 1, MAX
        out.append(w)
    return out


def extremes_hit(p: R.Problem, weights) -> bool:
    """some matching term weighs 1 and some weighs MAX"""
    lo = hi = False
    for cl, w in zip(p.clauses, weights):
        if w is None:
            continue
        used = np.intersect1d(cl.q_ci, cl.ind_ci)
        lo, hi = lo or bool((w[used] == 1).any()), hi or bool((w[used] == MAX).any())
    return lo and hi


def weighted_matches(p: R.Problem, weights) -> List[np.ndarray]:
    """M_c(q, i) = sum of w_c[h] over h in T_c(q) ^ I_c(i), int64 [n_queries, n_items] per clause"""
    out = []
    for cl, w in zip(p.clauses, weights):
        eff = np.full(cl.n_cols, ONE, np.int64) if w is None else np.clip(np.asarray(w).astype(np.int64), 1, MAX)
        t = sp.csr_matrix((eff[cl.q_ci], cl.q_ci, cl.q_rp), shape=(p.n_queries, cl.n_cols))
        i = sp.csr_matrix((np.ones(cl.ind_ci.size, np.int64), cl.ind_ci, cl.ind_rp), shape=(p.n_items, cl.n_cols))
        out.append(np.asarray((t @ i.T).todense(), dtype=np.int64))
    return out


def fold(boosts, matches) -> np.ndarray:
    """the f64 fold of D20 over integer match sums, clauses in call order"""
    score = np.zeros(matches[0].shape if matches else (0, 0), np.float64)
    for b, m in zip(boosts, matches):
        score = score + np.float64(b) * (m.astype(np.float64) * UNIT)
    return score


class Weighted:
    """A problem with one set of weights: the dense scores and the item orders, computed once and left unchanged."""

    def __init__(self, p: R.Problem, weights):
        assert len(weights) == len(p.clauses)
        self.p, self.weights = p, list(weights)
        self.m = weighted_matches(p, weights)
        self.score = fold([cl.boost for cl in p.clauses], self.m) if p.clauses else np.zeros((p.n_queries, p.n_items))
        plain = R.scores_of(p, np.arange(p.n_queries))
        assert np.array_equal(self.score > 0, plain > 0), "weights are >= 1: the positives are those of the unweighted score"
        self.order: Dict[bool, np.ndarray] = {}

    def order_of(self, use_fill: bool) -> np.ndarray:
        if use_fill not in self.order:
            p = self.p
            pos = np.arange(p.n_items)
            if use_fill:
                pos = np.empty(p.n_items, np.int64)
                pos[p.fill_order] = np.arange(p.n_items)
            self.order[use_fill] = np.lexsort((np.broadcast_to(pos, self.score.shape), -self.score), axis=-1)
        return self.order[use_fill]


def brute_force(wp: Weighted, rules: Sequence[RR.Rule], num, use_excl=True, use_mask=True, use_fill=True, no_backfill=False):
    """(count, idx, score, candidates, backfill steps) by the definition"""
    p, score = wp.p, wp.score
    nq = p.n_queries
    order = wp.order_of(bool(use_fill))
    ok = np.broadcast_to(p.mask != 0 if use_mask else np.ones(p.n_items, bool), score.shape).copy()
    if use_excl:
        ok[np.repeat(np.arange(nq), np.diff(p.excl_rp)), p.excl_ci] = False
    for r in rules:
        ok &= r.ok
    positive = ok & (score > 0)
    cand = int(np.count_nonzero(positive))
    steps = 0
    if not no_backfill:
        zero = ok & ~(score > 0)
        by_pos = zero[:, p.fill_order] if use_fill else zero
        need = num - np.minimum(positive.sum(1), num)
        reached = np.cumsum(by_pos, 1) >= need[:, None]
        per_query = np.where(reached.any(1), reached.argmax(1) // STEP + 1, -(-p.n_items // STEP))
        steps = int(per_query[need > 0].sum())
    take_from = positive if no_backfill else ok
    ok_sorted = np.take_along_axis(take_from, order, 1)
    rank = np.cumsum(ok_sorted, 1) - 1
    take = ok_sorted & (rank < num)
    count = take.sum(1).astype(np.int32)
    idx = np.full((nq, num), -1, np.int32)
    sc = np.zeros((nq, num), np.float64)
    r_, c_ = np.nonzero(take)
    idx[r_, rank[r_, c_]] = order[r_, c_]
    sc[r_, rank[r_, c_]] = score[r_, order[r_, c_]]
    return count, idx, sc, cand, steps


class DeviceWeighted:
    """The weight arrays on the session's device next to a recommend_ref.DeviceProblem (and, optionally, a recommend_rules_ref.DeviceRules)."""

    def __init__(self, dp: R.DeviceProblem, wp: Weighted, dr: Optional[RR.DeviceRules] = None):
        self.dp, self.wp, self.dr = dp, wp, dr
        self.dev = [None if w is None else R._dev(dp.sess, np.asarray(w, np.uint32)) for w in wp.weights]

    def run(self, names: Optional[Sequence[str]], num, use_excl=True, use_mask=True, use_fill=True, no_backfill=False, weights="own"):
        """names: the rules (None or () = none).  weights: "own", or an explicit list / None for DeviceSession.recommend."""
        dp = self.dp
        count, idx, score, stats = dp.sess.recommend(dp.n_queries, dp.p.n_items, dp.clauses, num, dp.excl if use_excl else None, dp.mask if use_mask else None,
                                                     dp.fill if use_fill else None, _lib.REC_NO_BACKFILL if no_backfill else 0,
                                                     rules=[self.dr.dev[n] for n in names] if names else None, weights=self.dev if weights == "own" else weights)
        dp.sess.synchronize()
        return count.cpu().numpy(), idx.cpu().numpy(), score.cpu().numpy(), stats.cpu().numpy()


def compare(got, want, tag=""):
    """counts, ids and score bits of two (count, idx, score, ...) results"""
    count, idx, score = got[:3]
    r_count, r_idx, r_score = want[:3]
    assert np.array_equal(count, r_count), f"{tag}: counts differ at queries {np.nonzero(count != r_count)[0][:10]}"
    live = np.arange(idx.shape[1])[None, :] < r_count[:, None]
    bad = np.nonzero(((idx != r_idx) & live).any(1))[0]
    assert bad.size == 0, f"{tag}: ids differ at queries {bad[:10]}: {idx[bad[0]][:r_count[bad[0]]]} vs {r_idx[bad[0]][:r_count[bad[0]]]}"
    assert np.array_equal(score[live].view(np.int64), r_score[live].view(np.int64)), f"{tag}: scores differ (bitwise)"


def check(dw: DeviceWeighted, names: Sequence[str], num, use_excl=True, use_mask=True, use_fill=True, no_backfill=False, lds_limit=_lib.REC_LDS_LIMIT):
    """Runs the weighted call under the named rules and compares count, ids, score bits and stats[0..4] with the restatement.  Returns the statistics."""
    p = dw.dp.p
    got = dw.run(names, num, use_excl, use_mask, use_fill, no_backfill)
    want = brute_force(dw.wp, [dw.dr.rules[n] for n in names], num, use_excl, use_mask, use_fill, no_backfill)
    tag = f"rules {list(names)} num {num} excl {use_excl} mask {use_mask} fill {use_fill} no_backfill {no_backfill}"
    compare(got, want, tag)
    stats = got[3]
    w = R.work_bound(p, use_excl)
    n_lds = int(np.count_nonzero(w <= lds_limit))
    assert stats[2] == 0, "candidate table overflow reported"
    assert (int(stats[0]), int(stats[1])) == (n_lds, dw.dp.n_queries - n_lds), f"{tag}: class split {stats[:2]} vs {(n_lds, dw.dp.n_queries - n_lds)}"
    assert int(stats[3]) == want[3], f"{tag}: candidates {stats[3]} vs {want[3]}"
    assert int(stats[4]) == (want[4] if names else 0), f"{tag}: backfill steps {stats[4]} vs {want[4]}"
    assert not stats[5:].any()
    return stats


def one_item_problem(n_items: int, n_terms: int, item: int, extra_queries: int = 0) -> R.Problem:
    """The counter bounds: one clause of n_terms columns, each listing the one item `item`; query 0 holds every column (w(q) = n_terms, no exclusions), the
    extra queries hold the first column alone.  No mask, the identity as fill_order."""
    irp = np.zeros(n_items + 1, np.int64)
    irp[item + 1:] = n_terms
    nq = 1 + extra_queries
    q_rp = np.concatenate([[0], n_terms + np.arange(nq, dtype=np.int64)]).astype(np.int64)
    q_ci = np.concatenate([np.arange(n_terms), np.zeros(extra_queries, np.int64)]).astype(np.int32)
    cl = R.Clause(n_terms, 1.0, irp, np.arange(n_terms, dtype=np.int32), q_rp, q_ci)
    p = R.Problem(n_items, nq, [cl], np.zeros(nq + 1, np.int64), np.zeros(0, np.int32), np.ones(n_items, np.uint8), np.arange(n_items, dtype=np.int32))
    R.dense_matches(p)
    return p


TIE_WEIGHTS = np.array([3 * ONE // 2, ONE // 2, ONE], np.uint32)
TIE_SCORE = np.float64(R.TIE_BOOST) * np.float64(1.5)


def tie_problem(seed, n_items, n_listed, starts) -> R.Problem:
    """Ties between different term sets: recommend_ref.make_tie_problem's fill order, exclusions and listed items, but three columns that every query
    holds -- the listed items at even fill positions list column 0, those at odd ones columns 1 and 2.  Under TIE_WEIGHTS both kinds sum to M = 3 * ONE / 2,
    so every candidate scores TIE_SCORE and the whole cut is decided by the backfill position: rows fill_order[start .. start + num)."""
    t = R.make_tie_problem(seed, n_items, n_listed, starts)
    pos = np.empty(n_items, np.int64)
    pos[t.fill_order] = np.arange(n_items)
    cols = np.where(pos % 2 == 0, 1, 2) * (pos < n_listed)                # entries per item row
    irp = np.zeros(n_items + 1, np.int64)
    np.cumsum(cols, out=irp[1:])
    ici = np.zeros(int(irp[-1]), np.int32)
    odd = np.nonzero(cols == 2)[0]
    ici[irp[odd]], ici[irp[odd] + 1] = 1, 2
    nq = len(starts)
    cl = R.Clause(3, R.TIE_BOOST, irp, ici, 3 * np.arange(nq + 1, dtype=np.int64), np.tile(np.arange(3, dtype=np.int32), nq))
    p = R.Problem(n_items, nq, [cl], t.excl_rp, t.excl_ci, t.mask, t.fill_order)
    R.dense_matches(p)
    return p


def check_ties(sess, p: R.Problem, starts, split, lds_limit=_lib.REC_LDS_LIMIT):
    """A tie_problem through check for num = 1, 20, 256; split = (LDS, global) queries."""
    wp = Weighted(p, [TIE_WEIGHTS])
    assert np.unique(wp.m[0][wp.m[0] > 0]).tolist() == [3 * ONE // 2] and set(np.diff(p.clauses[0].ind_rp).tolist()) >= {1, 2}
    dw = DeviceWeighted(R.DeviceProblem(sess, p), wp)
    for num in (1, 20, 256):
        stats = check(dw, (), num, lds_limit=lds_limit)
        assert (int(stats[0]), int(stats[1])) == split, stats
        count, idx, score, _, _ = brute_force(wp, (), num)
        assert (count == num).all() and np.array_equal(idx, np.stack([p.fill_order[s:s + num] for s in starts])) and (score == TIE_SCORE).all()
