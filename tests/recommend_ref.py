"""Shared by the recommendation tests: seeded problems for urcco_dev_recommend and its brute-force restatement.

The restatement is the scoring contract of DESIGN.md D15 word for word: per clause the dense integer matrix m_c = T_c I_c' of the 0/1
matrices, score = ((0.0 + boost_0 m_0) + boost_1 m_1) + ... in a Python loop over the clauses (float64, one rounding per step),
eligibility (exclusion row, item mask), np.lexsort on (backfill position, -score), the cut to num.  Counts, ids AND scores are
compared for exact equality: the m_c are integers and the sum has a fixed order, so there is no tolerance to choose."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import scipy.sparse as sp
import torch

from universal_recommender_amd import _lib


@dataclass
class Clause:
    n_cols: int
    boost: float
    ind_rp: np.ndarray   # CSR of the indicator matrix I_c (n_items x n_cols)
    ind_ci: np.ndarray
    q_rp: np.ndarray     # CSR of the query terms T_c (n_queries x n_cols), sorted unique columns
    q_ci: np.ndarray


@dataclass
class Problem:
    n_items: int
    n_queries: int
    clauses: List[Clause]
    excl_rp: np.ndarray
    excl_ci: np.ndarray
    mask: np.ndarray         # uint8 [n_items]
    fill_order: np.ndarray   # int32 permutation
    m: List[np.ndarray] = field(default_factory=list)   # dense m_c per clause (int64 [n_queries, n_items]), filled once by dense_matches
    cache: dict = field(default_factory=dict)           # brute_force: (scores, item order) per clause list


def _rows_to_csr(rows, dtype=np.int32):
    rp = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    ci = np.concatenate(rows).astype(dtype) if len(rows) and rp[-1] else np.zeros(0, dtype)
    return rp, ci


def random_rows(rng, n_rows, n_cols, lo, hi, sort=True):
    """n_rows rows of (at most) lo..hi distinct columns each (duplicates of a draw collapse)."""
    deg = np.minimum(rng.integers(lo, hi + 1, n_rows), n_cols)
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), deg)
    key = np.unique(rows * n_cols + rng.integers(0, n_cols, rows.size))
    out = np.split(key % n_cols, np.searchsorted(key // n_cols, np.arange(1, n_rows)))
    return [r if sort else rng.permutation(r) for r in out]


def make_problem(seed, n_items, n_queries, cols, boosts, k, hist_hi, hub_cols=(), hub_frac=1.0, hub_query_frac=0.25, long_row=0, excl_hi=8,
                 mask_frac=0.2, empty_query_frac=0.05, reverse_fill=False) -> Problem:
    """cols[c] / boosts[c]: the clauses.  hub_cols: columns of clause 0 that a fraction hub_frac of ALL item rows list (a query holding one touches
    most of the catalogue: the global class) -- a fraction hub_query_frac of the queries hold every hub column.  long_row: terms of one extra-long
    history row (clause 0).  The first empty_query_frac of the queries have no terms at all; the next three exclude all items but 0, 1 and 2 (fewer eligible
    items than num); the query that owns the strongest candidate of the whole batch has it in its exclusion row."""
    rng = np.random.default_rng(seed)
    clauses = []
    n_empty = max(int(n_queries * empty_query_frac), 1)
    for c, (nc, b) in enumerate(zip(cols, boosts)):
        ind = random_rows(rng, n_items, nc, 0, min(k, nc))
        if c == 0 and len(hub_cols):
            for i in range(n_items):
                if rng.random() < hub_frac:
                    ind[i] = np.union1d(ind[i], np.asarray(hub_cols))
        q = random_rows(rng, n_queries, nc, 0, min(hist_hi, nc))
        if c == 0:
            for r in range(n_queries):
                if len(hub_cols) and rng.random() < hub_query_frac:
                    q[r] = np.union1d(q[r], np.asarray(hub_cols))
                else:
                    q[r] = np.setdiff1d(q[r], np.asarray(hub_cols, dtype=np.int64))
            if long_row:
                q[min(n_empty, n_queries - 1)] = np.sort(rng.choice(np.setdiff1d(np.arange(nc), np.asarray(hub_cols, dtype=np.int64)), min(long_row, nc - len(hub_cols)), replace=False))
        for r in range(n_empty):
            q[r] = np.zeros(0, np.int64)
        irp, ici = _rows_to_csr(ind)
        qrp, qci = _rows_to_csr(q)
        clauses.append(Clause(nc, float(b), irp, ici, qrp, qci))
    mask = (rng.random(n_items) >= mask_frac).astype(np.uint8)
    fill = np.arange(n_items, dtype=np.int32)[::-1].copy() if reverse_fill else rng.permutation(n_items).astype(np.int32)
    excl = random_rows(rng, n_queries, n_items, 0, excl_hi, sort=False)
    p = Problem(n_items, n_queries, clauses, np.zeros(n_queries + 1, np.int64), np.zeros(0, np.int32), mask, fill)
    dense_matches(p)
    # the query with the strongest candidate of all excludes it; three queries exclude (nearly) everything
    if clauses:
        s = scores_of(p, np.arange(n_queries))
        s[:, mask == 0] = -1.0
        s[: n_empty + 3] = -1.0
        q = int(np.argmax(s.max(1)))
        excl[q] = np.union1d(excl[q], [int(np.argmax(s[q]))])
    for q in range(n_empty, min(n_empty + 3, n_queries)):
        keep = rng.choice(n_items, min(q - n_empty, n_items), replace=False)   # 0, 1, 2 items left
        excl[q] = rng.permutation(np.setdiff1d(np.arange(n_items), keep))
    p.excl_rp, p.excl_ci = _rows_to_csr(excl)
    return p


TIE_BOOST = 1.05


def make_tie_problem(seed, n_items, n_listed, starts) -> Problem:
    """Ties at the cut: one clause with one column (boost TIE_BOOST) that the first n_listed items of a random fill_order list and every query holds;
    query q excludes the items at fill positions 0 .. starts[q] - 1 (in shuffled order); the mask is all ones.  Every candidate scores exactly TIE_BOOST,
    so the whole cut is decided in the position digits of the selection key: with fill_order the rows are tie_rows(p, starts, num)."""
    rng = np.random.default_rng(seed)
    fill = rng.permutation(n_items).astype(np.int32)
    listed = np.zeros(n_items, bool)
    listed[fill[:n_listed]] = True
    irp = np.zeros(n_items + 1, np.int64)
    np.cumsum(listed, out=irp[1:])
    nq = len(starts)
    cl = Clause(1, TIE_BOOST, irp, np.zeros(n_listed, np.int32), np.arange(nq + 1, dtype=np.int64), np.zeros(nq, np.int32))
    excl_rp, excl_ci = _rows_to_csr([rng.permutation(fill[:s]) for s in starts])
    p = Problem(n_items, nq, [cl], excl_rp, excl_ci, np.ones(n_items, np.uint8), fill)
    dense_matches(p)
    return p


def tie_rows(p: Problem, starts, num):
    """What brute_force must give for a make_tie_problem with fill_order on (starts[q] + num <= n_listed): (idx [nq, num], score [nq, num])."""
    return np.stack([p.fill_order[s:s + num] for s in starts]), np.full((len(starts), num), TIE_BOOST)


def dense_matches(p: Problem):
    """m_c(q, i) = |T_c(q) ^ I_c(i)| for every clause: the integer product of the 0/1 matrices (kept sparse until the product is formed)."""
    p.m = []
    for cl in p.clauses:
        t = sp.csr_matrix((np.ones(cl.q_ci.size, np.int64), cl.q_ci, cl.q_rp), shape=(p.n_queries, cl.n_cols))
        i = sp.csr_matrix((np.ones(cl.ind_ci.size, np.int64), cl.ind_ci, cl.ind_rp), shape=(p.n_items, cl.n_cols))
        p.m.append(np.asarray((t @ i.T).todense(), dtype=np.int64))
    return p.m


def scores_of(p: Problem, rows: np.ndarray, clause_ids=None, boosts=None) -> np.ndarray:
    cid = range(len(p.clauses)) if clause_ids is None else clause_ids
    score = np.zeros((len(rows), p.n_items), np.float64)
    for n, c in enumerate(cid):
        b = p.clauses[c].boost if boosts is None else boosts[n]
        score = score + np.float64(b) * p.m[c][rows].astype(np.float64)
    return score


def brute_force(p: Problem, num, use_excl, use_mask, use_fill, no_backfill, clause_ids=None, boosts=None):
    """(count [nq], idx [nq, num], score [nq, num], candidates) by the definition.  The lexsort on (position, -score) runs once per clause list
    and position rule over ALL items (cached on the problem and never changed); eligibility then strikes items out of that order, and the cut follows."""
    nq = p.n_queries
    key = (tuple(clause_ids) if clause_ids is not None else None, tuple(boosts) if boosts is not None else None, bool(use_fill))
    if key not in p.cache:
        score = scores_of(p, np.arange(nq), clause_ids, boosts)
        pos = np.arange(p.n_items)
        if use_fill:
            pos = np.empty(p.n_items, np.int64)
            pos[p.fill_order] = np.arange(p.n_items)
        order = np.lexsort((np.broadcast_to(pos, score.shape), -score), axis=-1)
        p.cache[key] = (score, order)
    score, order = p.cache[key]
    ok = np.broadcast_to(p.mask != 0 if use_mask else np.ones(p.n_items, bool), score.shape).copy()
    if use_excl:
        ok[np.repeat(np.arange(nq), np.diff(p.excl_rp)), p.excl_ci] = False
    cand = int(np.count_nonzero(ok & (score > 0)))
    if no_backfill:
        ok &= score > 0
    ok_sorted = np.take_along_axis(ok, order, 1)
    rank = np.cumsum(ok_sorted, 1) - 1
    take = ok_sorted & (rank < num)
    count = take.sum(1).astype(np.int32)
    idx = np.full((nq, num), -1, np.int32)
    sc = np.zeros((nq, num), np.float64)
    r, c = np.nonzero(take)
    idx[r, rank[r, c]] = order[r, c]
    sc[r, rank[r, c]] = score[r, order[r, c]]
    return count, idx, sc, cand


def work_bound(p: Problem, use_excl, clause_ids=None) -> np.ndarray:
    """w(q) = sum_c sum_{h in T_c(q)} len(column h of I_c) + exclusions of q: what bins a query into the LDS or the global class."""
    w = np.zeros(p.n_queries, np.int64)
    for c in (range(len(p.clauses)) if clause_ids is None else clause_ids):
        cl = p.clauses[c]
        col_len = np.bincount(cl.ind_ci, minlength=cl.n_cols)
        w += np.bincount(np.repeat(np.arange(p.n_queries), np.diff(cl.q_rp)), weights=col_len[cl.q_ci], minlength=p.n_queries).astype(np.int64)
    if use_excl:
        w += np.diff(p.excl_rp)
    return w


def _dev(sess, a: np.ndarray) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype)))
    if sess.device.type == "cpu":
        import helpers
        return helpers.guarded(t.clone())
    return t.to(sess.device)


class DeviceProblem:
    """The problem's arrays on the session's device; the indicator matrices as CSC with shuffled columns (order inside a column is unspecified)."""

    def __init__(self, sess, p: Problem, seed=7):
        rng = np.random.default_rng(seed)
        self.sess, self.p = sess, p
        self.clauses = []
        for cl in p.clauses:
            item_of = np.repeat(np.arange(p.n_items, dtype=np.int32), np.diff(cl.ind_rp))
            order = np.lexsort((rng.random(cl.ind_ci.size), cl.ind_ci))
            cp = np.zeros(cl.n_cols + 1, np.int64)
            np.cumsum(np.bincount(cl.ind_ci, minlength=cl.n_cols), out=cp[1:])
            self.clauses.append((cl.n_cols, cl.boost, _dev(sess, cp), _dev(sess, item_of[order]), _dev(sess, cl.q_rp), _dev(sess, cl.q_ci)))
        self.excl = (_dev(sess, p.excl_rp), _dev(sess, p.excl_ci))
        self.mask = _dev(sess, p.mask)
        self.fill = _dev(sess, p.fill_order)
        self.n_queries = p.n_queries

    def run(self, num, use_excl=True, use_mask=True, use_fill=True, no_backfill=False, clause_ids=None, boosts=None):
        cl = self.clauses if clause_ids is None else [self.clauses[c] for c in clause_ids]
        if boosts is not None:
            cl = [(c[0], b) + tuple(c[2:]) for c, b in zip(cl, boosts)]
        count, idx, score, stats = self.sess.recommend(self.n_queries, self.p.n_items, cl, num, self.excl if use_excl else None, self.mask if use_mask else None,
                                                       self.fill if use_fill else None, _lib.REC_NO_BACKFILL if no_backfill else 0)
        self.sess.synchronize()
        return count.cpu().numpy(), idx.cpu().numpy(), score.cpu().numpy(), stats.cpu().numpy()


def check(dp: DeviceProblem, num, use_excl=True, use_mask=True, use_fill=True, no_backfill=False, clause_ids=None, boosts=None, lds_limit=_lib.REC_LDS_LIMIT):
    """Runs the call and compares count, ids, scores (exactly) and the statistics with the restatement.  Returns the statistics."""
    p = dp.p
    count, idx, score, stats = dp.run(num, use_excl, use_mask, use_fill, no_backfill, clause_ids, boosts)
    r_count, r_idx, r_score, r_cand = brute_force(p, num, use_excl, use_mask, use_fill, no_backfill, clause_ids, boosts)
    assert np.array_equal(count, r_count), f"counts differ at queries {np.nonzero(count != r_count)[0][:10]}"
    live = np.arange(num)[None, :] < r_count[:, None]
    bad = np.nonzero(((idx != r_idx) & live).any(1))[0]
    assert bad.size == 0, f"ids differ at queries {bad[:10]}: {idx[bad[0]][:r_count[bad[0]]]} vs {r_idx[bad[0]][:r_count[bad[0]]]}"
    assert np.array_equal(score[live].view(np.int64), r_score[live].view(np.int64)), "scores differ (bitwise)"
    w = work_bound(p, use_excl, clause_ids)
    n_lds = int(np.count_nonzero(w <= lds_limit))
    assert stats[2] == 0, "candidate table overflow reported"
    assert (int(stats[0]), int(stats[1])) == (n_lds, dp.n_queries - n_lds), f"class split {stats[:2]} vs {(n_lds, dp.n_queries - n_lds)}"
    assert int(stats[3]) == r_cand and not stats[4:].any()
    return stats


def check_ties(dp: DeviceProblem, starts, split, lds_limit=_lib.REC_LDS_LIMIT):
    """A make_tie_problem through check for num = 1, 20, 256 with fill_order; the restatement's rows are tie_rows; split = (LDS, global) queries."""
    for num in (1, 20, 256):
        stats = check(dp, num, lds_limit=lds_limit)
        assert (int(stats[0]), int(stats[1])) == split, stats
        r_count, r_idx, r_score, _ = brute_force(dp.p, num, True, True, True, False)
        idx, score = tie_rows(dp.p, starts, num)
        assert (r_count == num).all() and np.array_equal(r_idx, idx) and np.array_equal(r_score, score)
