"""Numpy restatement of decision D18 (include/urcco.h urcco_dev_item_*): the term rows of a batch of item queries, cut from the indicator
matrices.  Written from the decision text, not from the kernels; the yardstick of tests/test_sim_items.py and tests/test_gpu_items.py.

    row            the item's stored indicator list for the event type, n entries in stored order
    window         all n entries when n <= max_terms, else the first max_terms - 1
    term row       the distinct columns of the window inside 0..n_cols, ascending
    unknown item   (< 0 or >= n_items) empty rows
"""
from dataclasses import dataclass
from typing import List

import numpy as np
import torch

PLANTED = (0, 1, 2, 63, 64, 65, 4095, 4096, 4097)   # both sides of the wave / block and the block / global boundary
LONGEST = 5003
CAPS = (1, 2, 64, 65, 100, 4096, 4097, 6000)
N_ITEMS = 320
SENTINEL = -77


@dataclass
class Matrix:
    n_cols: int
    row_ptr: np.ndarray   # int64 [n_items + 1]
    col_idx: np.ndarray   # int32, stored order


@dataclass
class Problem:
    n_items: int
    mats: List[Matrix]
    q_items: np.ndarray   # int32


def window_len(n, cap):
    return n if n <= cap else cap - 1


def rows_ref(p: Problem, caps):
    """terms[t][q]: sorted unique int arrays"""
    terms = []
    for m, cap in zip(p.mats, caps):
        rows = []
        for i in p.q_items:
            row = m.col_idx[m.row_ptr[i]:m.row_ptr[i + 1]] if 0 <= i < p.n_items else m.col_idx[:0]
            w = row[: window_len(row.size, cap)]
            rows.append(np.unique(w[(w >= 0) & (w < m.n_cols)]))
        terms.append(rows)
    return terms


def windows(p: Problem, caps):
    """per type: (the rows' lengths n, the window lengths) of every query"""
    out = []
    for m, cap in zip(p.mats, caps):
        n = np.array([m.row_ptr[i + 1] - m.row_ptr[i] if 0 <= i < p.n_items else 0 for i in p.q_items], np.int64)
        out.append((n, np.where(n <= cap, n, cap - 1)))
    return out


def want_stats(p: Problem, caps, served=None):
    st = np.zeros(8, np.int64)
    for t, (n, w) in enumerate(windows(p, caps)):
        ok = served[t] if served is not None else np.ones(n.size, bool)
        st[0] += np.count_nonzero(ok & (w <= 64))
        st[1] += np.count_nonzero(ok & (w > 64) & (w <= 4096))
        st[2] += np.count_nonzero(ok & (w > 4096))
        st[3] += np.count_nonzero(ok & (n > caps[t]))
        st[6] += np.count_nonzero(~ok)
    return st


def make_problem(seed=9, n_items=N_ITEMS, cols=(9000, 300, 7000), stored=(9000, 520, 7000)):
    """Three event types with different n_cols; type 1 stores columns up to `stored[1]` > its n_cols and a few negative ones: entries outside 0..n_cols.
    Planted row lengths on both sides of every class boundary (type 0: all of PLANTED and LONGEST; type 1: up to 4097, so its long rows repeat columns;
    type 2: PLANTED), the other rows 0..30 entries.  Stored order is shuffled; duplicates are planted in short rows, block-class rows and the longest.
    Queries: every item, -1, n_items, n_items + 7 and repeats, shuffled."""
    rng = np.random.default_rng(seed)
    mats = []
    for t, (n_cols, hi) in enumerate(zip(cols, stored)):
        lens = rng.integers(0, 31, n_items)
        plant = list(PLANTED) + ([LONGEST] if t == 0 else [])
        who = rng.permutation(n_items)[: len(plant)]
        lens[who] = plant
        rows = []
        for i, n in enumerate(lens):
            row = rng.choice(hi, n, replace=n > hi).astype(np.int32)          # distinct where the columns allow it, in no order
            dup = n >= 2 and (i % 5 == 0 or n in (63, 65, 4095, 4096, LONGEST))
            if dup:                                                             # copies of earlier entries at random places
                k = max(1, n // 7)
                row[rng.permutation(n)[:k]] = row[rng.integers(0, n, k)]
            if t == 1 and n >= 3:
                row[rng.integers(0, n)] = -1 - int(rng.integers(0, 3))
            rows.append(row)
        rp = np.zeros(n_items + 1, np.int64)
        np.cumsum(lens, out=rp[1:])
        mats.append(Matrix(n_cols, rp, np.concatenate(rows).astype(np.int32)))
    q_items = np.concatenate([np.arange(n_items), [-1, n_items, n_items + 7], rng.integers(0, n_items, 77)]).astype(np.int32)
    return Problem(n_items, mats, q_items[rng.permutation(q_items.size)])


class DeviceProblem:
    def __init__(self, sess, p: Problem):
        self.sess, self.p = sess, p
        self.q_items = self._put(p.q_items)
        self.mats = [(m.n_cols, self._put(m.row_ptr), self._put(m.col_idx)) for m in p.mats]

    def _put(self, a):
        if a.size == 0:
            a = np.zeros(1, a.dtype)
        t = self.sess.empty(a.size, torch.from_numpy(a[:0].copy()).dtype)     # the session's allocator: guarded under HIPSIM_GUARD
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return t

    def specs(self, caps):
        return [(n_cols, cap, rp, ci) for (n_cols, rp, ci), cap in zip(self.mats, caps)]


def csr_rows(rp, ci):
    rp = rp.cpu().numpy()
    ci = ci.cpu().numpy()
    return rp, [ci[rp[i]:rp[i + 1]] for i in range(rp.size - 1)]


def check(d: DeviceProblem, caps, want=None):
    """Runs item_rows and asserts exact equality with the restatement: every term row, the final row_ptr, the bounds (= the window lengths), the
    statistics.  Returns (stats, rows) -- the device rows as numpy."""
    p = d.p
    rows, info = d.sess.item_rows(d.q_items, d.specs(caps), stats=True, n_items=p.n_items, keep_bounds=True)
    d.sess.synchronize()
    want = want if want is not None else rows_ref(p, caps)
    got = []
    for t, ((rp_t, ci_t), (_, w)) in enumerate(zip(rows, windows(p, caps))):
        rp, r = csr_rows(rp_t, ci_t)
        assert np.array_equal(rp, np.concatenate([[0], np.cumsum([x.size for x in want[t]])])), f"type {t}: final row_ptr differs"
        for q, (g, x) in enumerate(zip(r, want[t])):
            assert np.array_equal(g, x), f"type {t}, query {q} (item {p.q_items[q]}): {g[:20]} != {x[:20]}"
        assert np.array_equal(np.diff(info["bound_row_ptr"][t].cpu().numpy()), w), f"type {t}: the bounds are not the window lengths"
        assert info["bounds"][t] == w.sum()
        got.append(r)
    stats = info["stats"].cpu().numpy()
    assert np.array_equal(stats, want_stats(p, caps)), (stats, want_stats(p, caps))
    return stats, got


# ---- the capacity contract of urcco_dev_item_rows ------------------------------------------------------------------------------------------------
def rows_with_capacity(d: DeviceProblem, caps, capacity):
    """urcco_dev_item_bounds, then urcco_dev_item_rows with the capacities capacity(t, bound_row_ptr), through ctypes.  The col_idx arrays hold
    max(capacity, 1) entries from the session's allocator (under HIPSIM_GUARD a write past them faults), filled with SENTINEL."""
    from universal_recommender_amd import _lib
    s, p = d.sess, d.p
    nq, nt = d.q_items.numel(), len(p.mats)
    arr = (_lib.ItemEvent * nt)()
    rps = [s.empty(nq + 1, torch.int64) for _ in range(nt)]
    for t, (n_cols, cap, irp, ici) in enumerate(d.specs(caps)):
        arr[t].n_cols, arr[t].max_terms, arr[t].ind_row_ptr, arr[t].ind_col_idx, arr[t].term_row_ptr = n_cols, cap, irp.data_ptr(), ici.data_ptr(), rps[t].data_ptr()
    args = (s.handle, nq, d.q_items.data_ptr(), p.n_items, arr, nt)
    assert s.lib.urcco_dev_item_bounds(*args) == _lib.OK
    s.synchronize()
    bound = [rp.cpu().numpy().copy() for rp in rps]
    capacities = [int(capacity(t, bound[t])) for t in range(nt)]
    cis = []
    for t, c in enumerate(capacities):
        ci = s.empty(max(c, 1), torch.int32)
        ci.fill_(SENTINEL)
        cis.append(ci)
        arr[t].term_col_idx, arr[t].term_capacity = ci.data_ptr(), c
    st = s.empty(_lib.HIST_STATS_LEN, torch.int64)
    assert s.lib.urcco_dev_item_rows(*args, st.data_ptr()) == _lib.OK
    s.synchronize()
    return bound, capacities, [rp.cpu().numpy() for rp in rps], [ci.cpu().numpy() for ci in cis], st.cpu().numpy()


def check_capacity(d: DeviceProblem, caps, capacity):
    """A row is served iff the END of its bound is within the capacity; served rows equal the restatement, the others are empty and counted in
    stats[6]; stats[0..5] count served rows only; nothing is written at or past the capacity.  Returns the number of rows dropped per type."""
    p = d.p
    bound, capacities, rps, cis, stats = rows_with_capacity(d, caps, capacity)
    want = rows_ref(p, caps)
    served, dropped = [], []
    for t in range(len(p.mats)):
        ok = bound[t][1:] <= capacities[t]
        assert (np.diff(ok.astype(int)) <= 0).all()                           # the bound ends ascend: the served rows are a prefix
        lens = np.array([w.size if k else 0 for w, k in zip(want[t], ok)], np.int64)
        assert np.array_equal(rps[t], np.concatenate([[0], np.cumsum(lens)])), f"type {t}: the final row_ptr is not the scan of the served rows' lengths"
        for q, (w, k) in enumerate(zip(want[t], ok)):
            g = cis[t][rps[t][q]:rps[t][q + 1]]
            assert np.array_equal(g, w if k else w[:0]), f"type {t}, query {q}, served {k}: {g[:20]} != {w[:20]}"
        assert (cis[t][capacities[t]:] == SENTINEL).all(), f"type {t}: written at or past the capacity {capacities[t]}"
        served.append(ok)
        dropped.append(int(np.count_nonzero(~ok)))
    assert np.array_equal(stats, want_stats(p, caps, served)), (stats, want_stats(p, caps, served))
    return dropped


def capacity_cases(d: DeviceProblem, caps):
    """A cut at a middle query with block-class jobs on both sides of it; capacity 0 for one type only; every capacity one below its bound total."""
    p = d.p
    nq = p.q_items.size
    qm = nq // 2
    _, w0 = windows(p, caps)[0]
    if max(caps) > 64:
        assert (w0[:qm] > 64).any() and (w0[qm:] > 64).any()
    dropped = check_capacity(d, caps, lambda t, rp: rp[qm])
    assert all(x >= nq - qm for x in dropped), dropped
    dropped = check_capacity(d, caps, lambda t, rp: 0 if t == 1 else rp[-1])
    assert dropped[0] == 0 and dropped[1] > 0 and dropped[2] == 0, dropped
    dropped = check_capacity(d, caps, lambda t, rp: rp[-1] - 1)
    assert all(1 <= x < nq // 2 for x in dropped), dropped
