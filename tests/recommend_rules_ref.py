"""Shared by the rule tests: tests/recommend_ref.py's seeded problems extended with the inputs of urcco_dev_recommend_rules, and the brute force
extended with the rules (DESIGN.md decision D16).

Eligibility is a dense boolean [n_queries, n_items] computed by the definition: for ANY / NONE the sparse product of the two 0/1 matrices (> 0 /
== 0; entries of M outside 0..n_cols dropped, duplicates collapsed), for RANGE the comparison lo <= value < hi with INT64_MIN failing.  It is
and-ed into recommend_ref.brute_force's eligibility; the cached scores and the item order are shared with the rule-free tests and left unchanged.
stats[4] -- the backfill steps of 256 positions -- is restated from the same arrays.  Everything is compared for exact equality: counts, ids,
score bits, stats[0..4]; there is no tolerance to choose."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import scipy.sparse as sp

import recommend_ref as R
from universal_recommender_amd import _lib

NO_VALUE = np.iinfo(np.int64).min
OPEN_HI = np.iinfo(np.int64).max
N_VALUES = 40
STEP = 256   # positions per backfill step (REC_THREADS of csrc/cco_recommend.h)


@dataclass
class Rule:
    kind: int
    n_cols: int = 0
    m_rp: Optional[np.ndarray] = None    # ANY / NONE: CSR of M (n_items x n_cols) as stored: rows shuffled, duplicates and out-of-range columns allowed
    m_ci: Optional[np.ndarray] = None
    q_rp: Optional[np.ndarray] = None    # ANY / NONE: CSR of the query rows, sorted unique
    q_ci: Optional[np.ndarray] = None
    value: Optional[np.ndarray] = None   # RANGE: int64 [n_items], NO_VALUE = none
    lo: Optional[np.ndarray] = None      # RANGE: int64 [n_queries]
    hi: Optional[np.ndarray] = None
    ok: Optional[np.ndarray] = None      # dense eligibility [n_queries, n_items] by the definition, filled once by make_rules


def _eligibility(p: R.Problem, r: Rule) -> np.ndarray:
    if r.kind == _lib.RULE_RANGE:
        v = r.value[None, :]
        return (v != NO_VALUE) & (r.lo[:, None] <= v) & (v < r.hi[:, None])
    rows = np.repeat(np.arange(p.n_items), np.diff(r.m_rp))
    keep = (r.m_ci >= 0) & (r.m_ci < r.n_cols)
    m = sp.csr_matrix((np.ones(int(keep.sum()), np.int64), (rows[keep], r.m_ci[keep])), shape=(p.n_items, r.n_cols))
    m.data[:] = 1   # (the constructor summed the duplicates)
    t = sp.csr_matrix((np.ones(r.q_ci.size, np.int64), r.q_ci, r.q_rp), shape=(p.n_queries, r.n_cols))
    shared = np.asarray((t @ m.T).todense(), dtype=np.int64)
    return shared > 0 if r.kind == _lib.RULE_ANY else shared == 0


def make_rules(p: R.Problem, seed: int) -> Dict[str, Rule]:
    """{"any", "none", "range", "ind"}: the four rules of the tests over problem p (which needs at least two clauses).

    Property matrix n_items x 40, 0-4 values per item: value 0 is held by about 60 % of the items, value 39 by exactly three items (eligible under the
    mask, holding nothing else, dated in the middle of the date span: only an exclusion row can strike them); rows stored shuffled, one entry
    duplicated, one column of -1 and one of 40 (never a match).  "any": per query 0-2 values -- a tenth of the rows empty, a tenth {39} alone.
    "none": per query 0-2 values out of 1..38.  "range": item dates in ms, about 10 % NO_VALUE; per query [lo, hi) around the middle of the span, a
    fifth of the lower bounds and a fifth of the upper bounds open.  "ind": clause 1's indicator CSR as the matrix of an ANY rule against clause
    1's query rows -- the filter-bias form, rows of up to k unsorted entries."""
    rng = np.random.default_rng(seed)
    n, nq = p.n_items, p.n_queries
    rare = rng.choice(np.nonzero(p.mask)[0], 3, replace=False)
    rows: List[np.ndarray] = []
    for i in range(n):
        vals = rng.choice(np.arange(1, N_VALUES - 1), int(rng.integers(0, 4)), replace=False)
        if rng.random() < 0.6:
            vals = np.append(vals, 0)
        rows.append(rng.permutation(vals).astype(np.int64))
    for i in rare:
        rows[i] = np.array([N_VALUES - 1], np.int64)
    full = [i for i in range(n) if rows[i].size >= 2 and i not in rare]
    rows[full[0]] = np.append(rows[full[0]], rows[full[0]][0])           # a duplicated entry
    rows[full[1]] = rng.permutation(np.append(rows[full[1]], [-1, N_VALUES]))   # columns that never match
    m_rp, m_ci = R._rows_to_csr(rows)
    any_rows, none_rows = [], []
    for q in range(nq):
        u = rng.random()
        if u < 0.1:
            a = np.zeros(0, np.int64)
        elif u < 0.2:
            a = np.array([N_VALUES - 1], np.int64)
        else:
            a = rng.choice(np.arange(1, N_VALUES - 1), int(rng.integers(1, 3)), replace=False)
            if rng.random() < 0.5:
                a[0] = 0
        any_rows.append(np.unique(a).astype(np.int64))
        none_rows.append(np.unique(rng.choice(np.arange(1, N_VALUES - 1), int(rng.integers(0, 3)), replace=False)).astype(np.int64))
    a_rp, a_ci = R._rows_to_csr(any_rows)
    n_rp, n_ci = R._rows_to_csr(none_rows)
    t0, span = 1_700_000_000_000, 1_000_000_000
    value = t0 + rng.integers(0, span, n).astype(np.int64)
    value[rng.random(n) < 0.1] = NO_VALUE
    value[rare] = t0 + span // 2
    lo = t0 + rng.integers(0, int(0.45 * span), nq).astype(np.int64)
    hi = t0 + rng.integers(int(0.55 * span), span, nq).astype(np.int64)
    lo[rng.random(nq) < 0.2] = NO_VALUE       # open below: an item without a date still fails
    hi[rng.random(nq) < 0.2] = OPEN_HI
    c1 = p.clauses[1]
    ind_rows = [rng.permutation(c1.ind_ci[c1.ind_rp[i]:c1.ind_rp[i + 1]]).astype(np.int64) for i in range(n)]
    i_rp, i_ci = R._rows_to_csr(ind_rows)
    rules = {
        "any": Rule(_lib.RULE_ANY, N_VALUES, m_rp, m_ci, a_rp, a_ci),
        "none": Rule(_lib.RULE_NONE, N_VALUES, m_rp, m_ci, n_rp, n_ci),
        "range": Rule(_lib.RULE_RANGE, value=value, lo=lo, hi=hi),
        "ind": Rule(_lib.RULE_ANY, c1.n_cols, i_rp, i_ci, c1.q_rp, c1.q_ci),
    }
    for r in rules.values():
        r.ok = _eligibility(p, r)
    assert np.count_nonzero(m_ci == N_VALUES - 1) == 3 and 0.5 < np.mean([0 in r for r in rows]) < 0.7
    return rules


def brute_force(p: R.Problem, rules: Sequence[Rule], num, use_excl=True, use_mask=True, use_fill=True, no_backfill=False):
    """(count, idx, score, candidates, backfill steps, eligibility before the rules, eligibility) by the definition: recommend_ref.brute_force with the rules and-ed in."""
    nq = p.n_queries
    R.brute_force(p, 1, use_excl, use_mask, use_fill, no_backfill)     # fills the shared cache for this position rule (and never changes it)
    score, order = p.cache[(None, None, bool(use_fill))]
    base = np.broadcast_to(p.mask != 0 if use_mask else np.ones(p.n_items, bool), score.shape).copy()
    if use_excl:
        base[np.repeat(np.arange(nq), np.diff(p.excl_rp)), p.excl_ci] = False
    ok = base.copy()
    for r in rules:
        ok &= r.ok
    positive = ok & (score > 0)
    cand = int(np.count_nonzero(positive))
    # backfill steps: the walk over fill_order runs in steps of 256 positions until num results exist or the catalogue ends
    steps = 0
    if not no_backfill:
        zero = ok & ~(score > 0)
        by_pos = zero[:, p.fill_order] if use_fill else zero               # column = backfill position
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
    return count, idx, sc, cand, steps, base, ok


def assert_edge_cases(p: R.Problem, rules: Dict[str, Rule], lds_limit=_lib.REC_LDS_LIMIT, num=20):
    """What the problems must hold, asserted on the restatement alone (the three property rules together, every other input in use)."""
    rl = [rules["any"], rules["none"], rules["range"]]
    nq = p.n_queries
    count, idx, sc, _, _, base, ok = brute_force(p, rl, num)
    plain, _, _, _ = R.brute_force(p, num, True, True, True, False)
    score, _ = p.cache[(None, None, True)]
    short = (count > 0) & (count < num) & (plain == num)
    assert short.sum() >= 0.05 * nq, f"queries that end with 0 < count < num because of rules: {short.sum()} of {nq}"
    pos = np.empty(p.n_items, np.int64)
    pos[p.fill_order] = np.arange(p.n_items)
    skipped = walked_all = all_rejected = 0
    for q in range(nq):
        back = [int(i) for i, s in zip(idx[q, :count[q]], sc[q, :count[q]]) if s == 0.0]
        rejected = base[q] & ~ok[q]                                     # by the rules alone
        if back and (rejected & (pos < pos[back[-1]])).any():
            skipped += 1
        n_pos = int(np.count_nonzero(ok[q] & (score[q] > 0)))
        if n_pos < num and np.count_nonzero(ok[q] & ~(score[q] > 0)) < num - n_pos:
            walked_all += 1
        if (base[q] & (score[q] > 0)).any() and not (ok[q] & (score[q] > 0)).any():
            all_rejected += 1
    assert skipped >= 0.05 * nq, f"queries whose backfill skipped a rule-rejected position: {skipped} of {nq}"
    assert all_rejected >= 1, "a query with every positive rejected"
    assert walked_all >= 1, "a query that walks the whole catalogue"
    w = R.work_bound(p, True)
    assert (w <= lds_limit).any() and (w > lds_limit).any(), "both classes populated"


class DeviceRules:
    """The rules' arrays on the session's device, in the form DeviceSession.recommend takes."""

    def __init__(self, dp: R.DeviceProblem, rules: Dict[str, Rule]):
        self.dp, self.rules, self.dev = dp, rules, {}
        for name, r in rules.items():
            if r.kind == _lib.RULE_RANGE:
                self.dev[name] = (r.kind, R._dev(dp.sess, r.value), R._dev(dp.sess, r.lo), R._dev(dp.sess, r.hi))
            else:
                self.dev[name] = (r.kind, r.n_cols, R._dev(dp.sess, r.m_rp), R._dev(dp.sess, r.m_ci.astype(np.int32)), R._dev(dp.sess, r.q_rp),
                                  R._dev(dp.sess, r.q_ci.astype(np.int32)))

    def run(self, names: Optional[Sequence[str]], num, use_excl=True, use_mask=True, use_fill=True, no_backfill=False):
        """names = None: the rule-free entry point."""
        dp = self.dp
        count, idx, score, stats = dp.sess.recommend(dp.n_queries, dp.p.n_items, dp.clauses, num, dp.excl if use_excl else None, dp.mask if use_mask else None,
                                                     dp.fill if use_fill else None, _lib.REC_NO_BACKFILL if no_backfill else 0,
                                                     rules=None if names is None else [self.dev[n] for n in names])
        dp.sess.synchronize()
        return count.cpu().numpy(), idx.cpu().numpy(), score.cpu().numpy(), stats.cpu().numpy()


def check(dr: DeviceRules, names: Sequence[str], num, use_excl=True, use_mask=True, use_fill=True, no_backfill=False, lds_limit=_lib.REC_LDS_LIMIT):
    """Runs the call under the named rules and compares count, ids, score bits and stats[0..4] with the restatement.  Returns the statistics."""
    p = dr.dp.p
    count, idx, score, stats = dr.run(names, num, use_excl, use_mask, use_fill, no_backfill)
    r_count, r_idx, r_score, r_cand, r_steps, _, _ = brute_force(p, [dr.rules[n] for n in names], num, use_excl, use_mask, use_fill, no_backfill)
    tag = f"rules {list(names)} num {num} excl {use_excl} mask {use_mask} fill {use_fill} no_backfill {no_backfill}"
    assert np.array_equal(count, r_count), f"{tag}: counts differ at queries {np.nonzero(count != r_count)[0][:10]}"
    live = np.arange(num)[None, :] < r_count[:, None]
    bad = np.nonzero(((idx != r_idx) & live).any(1))[0]
    assert bad.size == 0, f"{tag}: ids differ at queries {bad[:10]}: {idx[bad[0]][:r_count[bad[0]]]} vs {r_idx[bad[0]][:r_count[bad[0]]]}"
    assert np.array_equal(score[live].view(np.int64), r_score[live].view(np.int64)), f"{tag}: scores differ (bitwise)"
    w = R.work_bound(p, use_excl)
    n_lds = int(np.count_nonzero(w <= lds_limit))
    assert stats[2] == 0, "candidate table overflow reported"
    assert (int(stats[0]), int(stats[1])) == (n_lds, dr.dp.n_queries - n_lds), f"{tag}: class split {stats[:2]} vs {(n_lds, dr.dp.n_queries - n_lds)}"
    assert int(stats[3]) == r_cand, f"{tag}: candidates {stats[3]} vs {r_cand}"
    assert int(stats[4]) == (r_steps if names else 0), f"{tag}: backfill steps {stats[4]} vs {r_steps}"
    assert not stats[5:].any()
    return stats
