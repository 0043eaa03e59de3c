"""urcco_dev_item_bounds / _rows on the host simulator (kernel LOGIC on the CPU) against the numpy restatement of decision D18 (tests/items_ref.py):
exact in every term row, final row_ptr, bound and statistic, for caps on both sides of every class boundary; the capacity clause; URCCO_BAD_ARG."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import items_ref as I
from universal_recommender_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def problem():
    return I.make_problem()


@pytest.fixture(scope="module")
def dev(sim_session, problem):
    return I.DeviceProblem(sim_session, problem)


@pytest.mark.parametrize("cap", I.CAPS)
def test_rows_match_the_restatement(dev, cap):
    stats, _ = I.check(dev, [cap] * 3)
    assert stats[0] + stats[1] + stats[2] == dev.p.q_items.size * 3 and stats[0] > 0, stats
    assert (stats[1] > 0) == (cap >= 65) and (stats[2] > 0) == (cap >= 4097), stats     # a window of 65 / 4097 entries needs a cap that admits it
    assert (stats[3] > 0) == (cap < I.LONGEST) and stats[4] == stats[5] == stats[6] == stats[7] == 0, stats


def test_mixed_caps(dev):
    stats, _ = I.check(dev, [6000, 2, 65])
    assert stats[0] > 0 and stats[1] > 0 and stats[2] > 0 and stats[3] > 0, stats
    I.check(dev, [1, 4097, 100])
    I.check(dev, [64])                       # one type alone


def test_problem_holds_the_edge_cases(problem):
    p = problem
    assert p.n_items == 320 and len({m.n_cols for m in p.mats}) == 3 and 380 <= p.q_items.size <= 420
    for t, m in enumerate(p.mats):
        n = np.diff(m.row_ptr)
        for c in I.PLANTED:
            assert (n == c).any(), (t, c)
        rows = [m.col_idx[m.row_ptr[i]:m.row_ptr[i + 1]] for i in range(p.n_items)]
        assert any(r.size > 3 and (np.diff(r) < 0).any() and (np.diff(r) > 0).any() for r in rows)                  # stored order is no sorted order
        dup = [r.size for r in rows if np.unique(r).size < r.size]
        assert any(s <= 64 for s in dup) and any(64 < s <= 4096 for s in dup), t                                    # duplicates in the wave and the block class
    m0, m1 = p.mats[0], p.mats[1]
    n0 = np.diff(m0.row_ptr)
    assert n0.max() == I.LONGEST and 4900 < I.LONGEST < 5100
    longest = m0.col_idx[m0.row_ptr[n0.argmax()]:m0.row_ptr[n0.argmax() + 1]]
    assert np.unique(longest).size < longest.size
    assert (m1.col_idx >= m1.n_cols).any() and (m1.col_idx < 0).any() and (m0.col_idx < m0.n_cols).all()           # the out-of-range clause is live
    # an out-of-range entry inside a cut window and one behind the cut: it counts toward the cut either way
    inside = behind = False
    for i in range(p.n_items):
        r = m1.col_idx[m1.row_ptr[i]:m1.row_ptr[i + 1]]
        bad = np.flatnonzero((r < 0) | (r >= m1.n_cols))
        if r.size > 64 and bad.size:
            inside |= bool((bad < 63).any())
            behind |= bool((bad >= 63).any())
    assert inside and behind
    q = p.q_items
    assert (q == -1).any() and (q == p.n_items).any() and (q == p.n_items + 7).any() and np.unique(q).size < q.size
    assert set(range(p.n_items)) <= set(q.tolist())
    # a term row shorter than its window because of duplicates, for a cut and an uncut row
    for cap in (64, 6000):
        want = I.rows_ref(p, [cap] * 3)
        w = I.windows(p, [cap] * 3)[0][1]
        assert any(r.size < x for r, x in zip(want[0], w))


def test_bad_arguments(dev):
    s = dev.sess
    lib = s.lib
    nq = dev.q_items.numel()
    ok = dev.specs([5] * 3)

    def call(specs=ok, n_types=None, rows=False, capacity=0, q_items=dev.q_items.data_ptr(), n_queries=nq, row_ptr=True, col_idx=True):
        arr = (_lib.ItemEvent * max(len(specs), 17))()
        keep = []
        for t, (n_cols, cap, irp, ici) in enumerate(specs):
            rp, ci = s.empty(nq + 1, torch.int64), s.empty(8, torch.int32)
            keep += [rp, ci]
            arr[t].n_cols, arr[t].max_terms = n_cols, cap
            arr[t].ind_row_ptr, arr[t].ind_col_idx = irp.data_ptr() if irp is not None else None, ici.data_ptr() if ici is not None else None
            arr[t].term_row_ptr, arr[t].term_col_idx, arr[t].term_capacity = rp.data_ptr() if row_ptr else None, ci.data_ptr() if col_idx else None, capacity
        n = len(specs) if n_types is None else n_types
        if rows:
            return lib.urcco_dev_item_rows(s.handle, n_queries, q_items, dev.p.n_items, arr, n, None)
        return lib.urcco_dev_item_bounds(s.handle, n_queries, q_items, dev.p.n_items, arr, n)

    assert call() == _lib.OK
    assert call(col_idx=False) == _lib.OK                                                               # _bounds does not read term_col_idx
    for rows in (False, True):
        assert call(n_types=0, rows=rows) == _lib.BAD_ARG
        assert call(specs=[ok[t % 3] for t in range(17)], rows=rows) == _lib.BAD_ARG                   # n_types > URCCO_REC_MAX_CLAUSES
        assert call(specs=[ok[0][:1] + (0,) + ok[0][2:]], rows=rows) == _lib.BAD_ARG                   # max_terms < 1
        assert call(specs=[(-1,) + ok[0][1:]], rows=rows) == _lib.BAD_ARG                              # n_cols < 0
        assert call(specs=[ok[0][:2] + (None, ok[0][3])], rows=rows) == _lib.BAD_ARG                   # a NULL the call needs
        assert call(specs=[ok[0][:3] + (None,)], rows=rows) == _lib.BAD_ARG
        assert call(q_items=None, rows=rows) == _lib.BAD_ARG
        assert call(row_ptr=False, rows=rows) == _lib.BAD_ARG
        assert call(n_queries=(1 << 31) // 3 + 1, rows=rows) == _lib.BAD_ARG                           # n_queries * n_types >= 2^31
    assert call(rows=True, col_idx=False) == _lib.BAD_ARG
    assert call(rows=True, capacity=-1) == _lib.BAD_ARG                                                # a negative capacity
    assert call(rows=True, capacity=-(1 << 40)) == _lib.BAD_ARG
    assert lib.urcco_version() == 305


def test_no_queries(sim_session, dev):
    rows, info = sim_session.item_rows(dev.q_items[:0], dev.specs([5] * 3), stats=True, n_items=dev.p.n_items)
    assert all(rp.tolist() == [0] for rp, _ in rows) and info["stats"].tolist() == [0] * 8 and info["bounds"] == [0] * 3


@pytest.mark.parametrize("cap", (64, 100, 6000))
def test_capacity_below_the_bounds(dev, cap):
    """Buffers of exactly max(capacity, 1) entries: under HIPSIM_GUARD a write past them faults."""
    I.capacity_cases(dev, [cap] * 3)


def test_two_runs_are_identical(dev):
    a, _ = dev.sess.item_rows(dev.q_items, dev.specs([100, 4097, 65]), n_items=dev.p.n_items)
    b, _ = dev.sess.item_rows(dev.q_items, dev.specs([100, 4097, 65]), n_items=dev.p.n_items)
    dev.sess.synchronize()
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1][: int(x[0][-1])], y[1][: int(y[0][-1])]) for x, y in zip(a, b))


def test_under_guard_pages():
    """This module once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument)."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    env = dict(os.environ, HIPSIM_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
