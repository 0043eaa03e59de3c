"""The two forms of the expand tables (cco_kernels.h, ExpandForm): narrow -- 32-bit B' row starts, the work prefix modulo 2^32 -- and the wide
fallback.  Same builds in both forms, on the host simulator and on hardware: equal row for row and equal to the oracle, with the form that ran
read back from the session, so a fallback that never triggers cannot pass.

Not covered here: a verdict from a ROW's work.  No consumer of the narrow prefix takes a difference wider than one chunk of an item row (the
multi-pass class sizes its passes from the 64-bit work array), so the library has no such test to trip; the tile-sum test is the one condition the
64-bit work depends on."""
import numpy as np
import pytest
import torch

from helpers import check_indicators, to_dev, to_params, rand_csr
from oracle import c_oracle as O
from universal_recommender_amd import device as D

SEED = 77
TILE = 2048  # urcco::SCAN_TILE


def _build(sess, mats, params, primary=None):
    """cross_occurrence_device with the form word read after every event type: ([DevIndicators], [form], a_col_ptr, a_row_idx, [B' row_ptr], primary).
    primary: the down-sampled A and its CSC of an earlier call (the order inside a CSC column is unspecified and differs from one transposition to the next)"""
    dm = [to_dev(m, sess.device) for m in mats]
    ps = to_params(params)
    if primary is None:
        raw = sess.column_counts(dm[0].col_idx, dm[0].nnz_bound, dm[0].n_cols)
        a, cnt_a = sess.downsample(dm[0], dm[0].nnz_bound, raw, SEED, ps[0].max_elements_per_row, 0)
        primary = (a, cnt_a) + tuple(sess.transpose(a, cnt_a))
    a, cnt_a, a_cp, a_ri = primary
    outs, forms, brp = [], [], []
    for d, (m, p) in enumerate(zip(dm, ps)):
        if d == 0:
            b, cnt_b = a, cnt_a
        else:
            b, cnt_b = sess.downsample(m, m.nnz_bound, sess.column_counts(m.col_idx, m.nnz_bound, m.n_cols), SEED, p.max_elements_per_row, 0)
        outs.append(sess.cco_rows(0, dm[0].n_cols, dm[0].n_cols, a_cp, a_ri, a.nnz_bound, b, cnt_a, cnt_b, dm[0].n_rows, d == 0, p))
        forms.append(sess.expand_form())
        brp.append(b.row_ptr.cpu().numpy())
    sess.synchronize()
    return outs, forms, a_cp.cpu().numpy(), a_ri.cpu().numpy(), brp, primary


def _same(x, y):
    for a, b in zip(x.to_host(), y.to_host()):
        assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
    assert np.array_equal(x.stats.cpu().numpy()[:30], y.stats.cpu().numpy()[:30])


def _three_forms(sess):
    rng = np.random.default_rng(5)
    mats = [rand_csr(rng, 2000, 300, 8), rand_csr(rng, 2000, 300, 12), rand_csr(rng, 2000, 40, 3)]
    params = [O.DatasetParams(100, 20, None)] * 3
    ref = O.cross_occurrence_downsampled(mats, params, SEED, 0, 1, 0, None)
    try:
        sess.set_expand_test(0, 0)
        narrow, f0, a_cp, a_ri, brp, primary = _build(sess, mats, params)
        assert f0 == [0, 0, 0], f0
        nnz = int(a_cp[-1])
        assert nnz > 4 * TILE  # several scan tiles; item rows start, end and run across their boundaries
        # the limit is a strict bound on every event type's largest tile sum (computed here from the very CSC the device built and keeps using)
        for d, rp in enumerate(brp):
            plen = np.diff(rp)[a_ri[:nnz]]
            tmax = int(np.concatenate([plen, np.zeros((-nnz) % TILE, np.int64)]).reshape(-1, TILE).sum(1).max())
            sess.set_expand_test(tmax + 1, 0)
            assert _build(sess, mats, params, primary)[1][d] == 0
            sess.set_expand_test(tmax, 0)
            assert _build(sess, mats, params, primary)[1][d] == 5
        sess.set_expand_test(1, 0)  # every tile with a pair in it reaches the limit
        wide, f1, *_ = _build(sess, mats, params)
        assert f1 == [5, 5, 5], f1  # FORM_WIDE | FORM_TILE
        # ... and the wide form for the other device-side reason left at toy size: no packed B' (the plain entry point)
        sess.set_expand_test(0, 0)
        sess.pack_counts = False
        plain, f2, *_ = _build(sess, mats, params)
        assert f2 == [17, 17, 17], f2  # FORM_WIDE | FORM_HOST
    finally:
        sess.pack_counts = True
        sess.set_expand_test(0, 0)
    for d in range(3):
        st = narrow[d].stats.cpu().numpy()
        assert int(st[0]) == ref[d].pairs and int(st[29]) == 0
        check_indicators(narrow[d].to_host(), ref[d])
        _same(narrow[d], wide[d])
        _same(narrow[d], plain[d])


def _ladder():
    """Item rows of exactly 1, 64 and 65 pairs and one per LDS class and the multi-pass class: item j is held by n users who each bring a B' row of
    length L with columns disjoint from the other users' -- work = distinct columns = n * L."""
    steps = [(1, 1), (1, 64), (1, 65), (5, 50), (5, 200), (10, 200), (10, 400), (20, 400), (35, 400)]  # 1, 64, 65, 250, 1000, 2000, 4000, 8000, 14000
    rng = np.random.default_rng(9)
    a_rows, b_rows = [], []
    for j, (n, L) in enumerate(steps):
        for t in range(n):
            a_rows.append(np.array([j], np.int64))
            b_rows.append(np.arange(t * L, (t + 1) * L, dtype=np.int64))
    n_items, n_cols = 40, 35 * 400
    for _ in range(400):  # background users on other items: counts above one, scores that differ
        a_rows.append(np.unique(rng.integers(len(steps), n_items, 3)))
        b_rows.append(np.unique(rng.integers(0, n_cols, 6)))

    def csr(rows, nc):
        rp = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=rp[1:])
        return O.Csr(len(rows), nc, rp, np.concatenate(rows).astype(np.int32))
    return [csr(a_rows, n_items), csr(b_rows, n_cols)], [O.DatasetParams(500, 20, None)] * 2


def _wrapped(sess):
    mats, params = _ladder()
    ref = O.cross_occurrence_downsampled(mats, params, SEED, 0, 1, 0, None)
    total = ref[1].pairs
    assert total > 30000
    try:
        # the prefix of the second event type runs from 2^32 - total / 2 to 2^32 + total / 2: the rows in the middle of the CSC straddle the wrap
        sess.set_expand_test(0, (1 << 32) - total // 2)
        outs, forms, a_cp, a_ri, brp, primary = _build(sess, mats, params)
        # the rows as built, not as designed: the per-row work the library itself computes on this CSC and this B' (narrow prefix, wrapped)
        a, _, d_cp, d_ri = primary
        work = sess.row_work(0, mats[0].n_cols, mats[0].n_cols, d_cp, d_ri, a.nnz_bound, outs[1].sampled_row_ptr).cpu().numpy()
        assert sess.expand_form() == 0
    finally:
        sess.set_expand_test(0, 0)
    assert forms == [0, 0], forms
    nnz = int(a_cp[-1])
    plen = np.diff(brp[1])[a_ri[:nnz]]
    pref = np.concatenate([[0], np.cumsum(plen)])
    assert np.array_equal(work, pref[a_cp[1:]] - pref[a_cp[:-1]])
    assert work[:9].tolist() == [1, 64, 65, 250, 1000, 2000, 4000, 8000, 14000]  # down-sampling left the designed rows whole
    assert np.diff(a_cp)[:3].tolist() == [1, 1, 1]                               # ... of one user each: exactly 1, 64 and 65 pairs
    # where the narrow prefix wraps: strictly inside the slice of the multi-pass row (item 8), whose chunks straddle it
    seed = (1 << 32) - total // 2
    row = int(np.searchsorted(seed + pref[a_cp], 1 << 32, side="right")) - 1
    assert row == 8 and seed + pref[a_cp[row]] < (1 << 32) < seed + pref[a_cp[row + 1]], (row, seed + pref[a_cp[row]], seed + pref[a_cp[row + 1]])
    st = outs[1].stats.cpu().numpy()
    assert int(st[0]) == total  # the 64-bit work of every row, rebuilt from tile bases + low words
    rows_per_bin = st[1:8]
    assert np.all(rows_per_bin > 0), rows_per_bin  # micro, the five LDS classes, multi-pass
    assert int(st[29]) == 0
    for d in range(2):
        check_indicators(outs[d].to_host(), ref[d])


def _row_work(sess):
    """The 64-bit work of every row, rebuilt from the scan's tile bases plus the low words of the narrow prefix, against numpy -- on a CSC whose columns
    start and end exactly on scan-tile boundaries (items 0, 1, 3, 6), run across them (2, 6) or sit right behind one (4, 7), with an empty column."""
    users = [2048, 2048, 3000, 1096, 1, 0, 4095, 1, 2000]
    a_cp = np.concatenate([[0], np.cumsum(users)]).astype(np.int64)
    assert a_cp[1] % TILE == 0 and a_cp[2] % TILE == 0 and a_cp[4] % TILE == 0 and a_cp[7] % TILE == 0 and a_cp[3] % TILE != 0
    nnz, n_users, n_items = int(a_cp[-1]), 5000, len(users)
    rng = np.random.default_rng(3)
    a_ri = rng.integers(0, n_users, nnz).astype(np.int32)
    b_rp = np.concatenate([[0], np.cumsum(rng.integers(0, 41, n_users))]).astype(np.int64)
    plen = np.diff(b_rp)[a_ri]
    pref = np.concatenate([[0], np.cumsum(plen)])
    ref = pref[a_cp[1:]] - pref[a_cp[:-1]]
    total = int(pref[-1])
    dev = sess.device
    t_cp, t_ri, t_rp = (torch.from_numpy(x).to(dev) for x in (a_cp, np.concatenate([a_ri, np.zeros(777, np.int32)]), b_rp))
    tmax = int(np.concatenate([plen, np.zeros((-nnz) % TILE, np.int64)]).reshape(-1, TILE).sum(1).max())
    try:
        # (limit, seed, form): production; the prefix wrapping at 2^32 in the middle of the CSC; the limit just above / at the largest tile sum
        for limit, seed, form in [(0, 0, 0), (0, (1 << 32) - total // 2, 0), (tmax + 1, (1 << 32) - 5, 0), (tmax, 0, 5), (tmax, (1 << 32) - total // 2, 5)]:
            sess.set_expand_test(limit, seed)
            for lo, hi in [(0, n_items), (2, 7)]:
                got = sess.row_work(lo, hi, n_items, t_cp, t_ri, nnz + 777, t_rp).cpu().numpy()
                assert sess.expand_form() == form, (limit, seed, sess.expand_form())
                assert np.array_equal(got, ref[lo:hi]), (limit, seed, lo, hi, got, ref[lo:hi])
    finally:
        sess.set_expand_test(0, 0)


def test_row_work_sim(sim_session):
    _row_work(sim_session)


@pytest.mark.gpu
def test_row_work_gpu(gpu_session):
    _row_work(gpu_session)


def test_three_forms_sim(sim_session):
    _three_forms(sim_session)


def test_wrapped_prefix_sim(sim_session):
    _wrapped(sim_session)


@pytest.mark.gpu
def test_three_forms_gpu(gpu_session):
    _three_forms(gpu_session)


@pytest.mark.gpu
def test_wrapped_prefix_gpu(gpu_session):
    _wrapped(gpu_session)
