"""Workloads and a plain-numpy model of the k11 = 1 prefilter of the packed row kernels (csrc/cco_rows.hip), shared by
test_sim_prefilter.py and test_gpu_prefilter.py.

A `crafted` build: item t of A is held by ca users who hold nothing else; their B' rows deal out the row's D distinct columns (fresh columns per item),
one user per column (k11 = 1) except the first `multi`, which two users share (k11 = 2).  Every column's count cB is then raised to its target by FILLER
users who hold no item of A -- their B' rows are never expanded, so a column count costs nothing in the simulator.  n_users is free: it only pads."""
import numpy as np
import torch

from oracle import c_oracle as O
from universal_recommender_amd import _lib

XLX_TABLE = 4096
CLAMP_BIN = 255


def zipf_counts(rng, n, cmax=400):
    """Counts of a row's candidate columns: columns are met in proportion to their count and counts fall like 1 / c^2, so the candidates' counts fall like
    1 / c, 1 .. cmax -- a tail beyond the clamp bin included."""
    c = np.arange(1, cmax + 1, dtype=np.float64)
    p = 1.0 / c
    return rng.choice(np.arange(1, cmax + 1), size=n, p=p / p.sum()).astype(np.int64)


def crafted(rng, sizes, ca, n_users, cb_of=zipf_counts, multi=5):
    """Returns ([A, B], rows): rows[t] = (ca, k11[D], cB[D]) of item t's candidates in A'B."""
    n_items = len(sizes)
    a_rows = [[t] for t in range(n_items) for _ in range(ca)]
    b_rows = [[] for _ in range(n_items * ca)]
    col0, rows, want = 0, [], []
    for t, D in enumerate(sizes):
        cb = np.maximum(cb_of(rng, D), 1)
        k11 = np.ones(D, np.int64)
        m = min(multi, D) if ca >= 2 else 0
        k11[:m] = 2
        cb = np.maximum(cb, k11)
        for j in range(D):
            u = t * ca + j % ca
            b_rows[u].append(col0 + j)
            if j < m:
                b_rows[t * ca + (j + 1) % ca].append(col0 + j)
        rows.append((ca, k11, cb))
        want.append(cb - k11)
        col0 += D
    want = np.concatenate(want)
    n_fill = int(want.max()) if want.size else 0
    first_fill = n_items * ca
    assert first_fill + n_fill <= n_users, "n_users too small for the fillers"
    fill_rows = [np.nonzero(want > f)[0] for f in range(n_fill)]   # filler f holds every column that needs more than f fillers
    lens_a = np.zeros(n_users, np.int64)
    lens_a[:first_fill] = 1
    a_rp = np.zeros(n_users + 1, np.int64)
    np.cumsum(lens_a, out=a_rp[1:])
    a = O.Csr(n_users, n_items, a_rp, np.array([r[0] for r in a_rows], np.int32))
    all_rows = [np.sort(np.array(r, np.int64)) for r in b_rows] + fill_rows
    lens_b = np.zeros(n_users, np.int64)
    lens_b[:len(all_rows)] = [r.size for r in all_rows]
    b_rp = np.zeros(n_users + 1, np.int64)
    np.cumsum(lens_b, out=b_rp[1:])
    b = O.Csr(n_users, col0, b_rp, np.concatenate(all_rows).astype(np.int32))
    return [a, b], rows


def llr_k11_1(sess, ca, cbs, n_users):
    """LLR of (k11 = 1, cA, cB) for every cB of `cbs` through the library under test (urcco_dev_llr: the general form, bit-identical to the tables)."""
    dev = sess.device
    cbs = np.asarray(cbs, np.int64)
    wa = torch.full((cbs.size,), int(ca), dtype=torch.int64, device=dev)
    wb = torch.from_numpy(cbs).to(dev)
    wab = torch.ones(cbs.size, dtype=torch.int64, device=dev)
    nu = torch.full((cbs.size,), int(n_users), dtype=torch.int64, device=dev)
    out = sess.llr(wa, wb, wab, nu)
    sess.synchronize()
    return out.cpu().numpy()


def mono_limit(sess, ca, n_users):
    """The monotone limit of cA re-derived from its definition: the largest m with, for all 1 <= cB < m, every operand of the table form of cB and cB + 1
    inside the tables, f(cB) > f(cB + 1) and f(cB) > 0; 0 when that fails at the start."""
    def in_tables(cb):
        k12, k21, d22 = ca - 1, cb - 1, ca + cb - 1
        return min(k12, k21) >= 0 and max(k12, k21, cb, d22) < XLX_TABLE and d22 <= n_users
    hi = 1
    while in_tables(hi + 1):
        hi += 1          # f(1 .. hi) can be evaluated in the tables
    if not in_tables(1) or hi < 2:
        return 0
    f = llr_k11_1(sess, ca, np.arange(1, hi + 1), n_users)
    ok = (f[:-1] > f[1:]) & (f[:-1] > 0.0)     # ok[c - 1]: the condition at cB = c, c < hi
    bad = np.nonzero(~ok)[0]
    m = int(bad[0]) + 1 if bad.size else hi
    return 0 if m <= 1 else m


def model_scored(rows, k, limit_of, exclude_self=False):
    """Candidates the score phase sees, per row, by the prefilter's rule: (scored, distinct)."""
    scored = distinct = 0
    for ca, k11, cb in rows:
        D = k11.size
        distinct += D
        need = k + (1 if exclude_self else 0)
        keep = D
        if D > need:
            one = k11 == 1
            hist = np.bincount(cb[one & (cb < CLAMP_BIN)], minlength=CLAMP_BIN)
            cum = np.cumsum(hist)
            at = np.nonzero(cum >= need)[0]
            lim = limit_of(ca)
            if at.size and at[0] < lim:
                keep = D - int((one & (cb > at[0]) & (cb <= lim)).sum())
        scored += keep
    return scored, distinct


def run_both(sess, mats, params, seed, run, bits=0):
    """The build with the prefilter and with it switched off: (on, off) outputs.  `run(sess, mats, params, seed)` -> per event type outputs."""
    sess.set_debug(bits)
    on = run(sess, mats, params, seed)
    sess.set_debug(bits | _lib.DBG_NO_PREFILTER)
    try:
        off = run(sess, mats, params, seed)
    finally:
        sess.set_debug(0)
    return on, off


def assert_bit_equal(on, off, as_sets=False):
    from helpers import sort_rows
    for d, (x, y) in enumerate(zip(on, off)):
        gx, gy = x.to_host(), y.to_host()
        if as_sets:
            gx, gy = sort_rows(gx), sort_rows(gy)
        assert np.array_equal(gx[0], gy[0]), f"event {d}: row lengths differ with the prefilter"
        assert np.array_equal(gx[1], gy[1]), f"event {d}: ids differ with the prefilter"
        assert np.array_equal(gx[2].view(np.int64), gy[2].view(np.int64)), f"event {d}: LLR bits differ with the prefilter"


def scored_and_distinct(sess, mats, params, seed, run):
    """stats[30] of every event type: (candidates scored, distinct candidates) -- two builds with stage timing on."""
    sess.set_timing(True)
    try:
        sess.set_debug(_lib.DBG_COUNT_SCORED)
        scored = [int(o.stats.cpu().numpy()[30]) for o in run(sess, mats, params, seed)]
        sess.set_debug(0)
        distinct = [int(o.stats.cpu().numpy()[30]) for o in run(sess, mats, params, seed)]
    finally:
        sess.set_debug(0)
        sess.set_timing(False)
    return scored, distinct
