"""urcco_dev_history_index / _bounds / _rows on the host simulator (kernel LOGIC on the CPU) against the numpy restatement of decision D17
(tests/history_ref.py): exact in every term row, exclusion row and final row_ptr, for caps on both sides of every class boundary.

The keys of the select, by byte: make_problem's times differ in the lowest time byte alone; make_key_problem lets each time byte 0..7 be the only
one that differs (positive and negative base, byte 7 across the sign bit), two bytes around uniform ones, the whole int64 domain with INT64_MIN / -1 /
0 / INT64_MAX planted, and equal times; the position bytes 0..2 differ throughout, make_far_problem adds the top one (positions on both sides of 2^24).
Clauses of include/urcco.h beyond the rows themselves: a capacity below the bound (served prefix, empty rows behind it, stats[6], stats[0..5] of the
served rows only, nothing written past the capacity -- the guard-page rerun faults on it) and URCCO_BAD_ARG for a negative capacity."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import history_ref as H
from universal_recommender_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def problem():
    return H.make_problem()


@pytest.fixture(scope="module")
def dev(sim_session, problem):
    return H.DeviceProblem(sim_session, problem)


def test_index_holds_every_users_positions(dev):
    for s, (_, rp, pos, *_rest) in zip(dev.p.streams, dev.ev):
        rp, rows = H.csr_rows(rp, pos)
        assert rp[-1] == np.count_nonzero(s.users >= 0)
        for u, r in enumerate(rows):
            assert np.array_equal(np.sort(r), np.flatnonzero(s.users == u))


@pytest.mark.parametrize("cap", H.CAPS)
def test_rows_match_the_restatement(dev, cap):
    stats, _, _ = H.check(dev, [cap] * 3)
    n_pairs = dev.p.q_users.size * 3
    assert stats[0] + stats[1] + stats[2] == n_pairs and stats[0] > 0 and stats[1] > 0 and stats[2] > 0, stats   # every class served pairs
    assert (stats[3] > 0) == (cap < H.HEAVY) and stats[4] > 0 and stats[5] > 0, stats


def test_mixed_caps_no_blacklist_no_extra(dev):
    H.check(dev, [100, 1, 3])
    _, _, excl = H.check(dev, [5, 5, 5], use_extra=False, blacklist=[False] * 3)
    assert all(r.size == 0 for r in excl)
    H.check(dev, [5, 64, 5000], use_extra=False, blacklist=[False, False, True])


def test_problem_holds_the_edge_cases(problem, dev):
    p = problem
    n_events = sum(s.users.size for s in p.streams)
    assert 35000 < n_events < 50000
    for t, s in enumerate(p.streams):
        n_u = np.array([r.size for r in dev.by_user[t]])
        for c in (0, 1, 63, 64, 65):
            assert (n_u == c).any(), (t, c)
        if t < 2:
            for c in (4095, 4096, 4097):
                assert (n_u == c).any(), (t, c)
    assert max(r.size for r in dev.by_user[0]) == H.HEAVY
    assert p.streams[1].times is None and (p.streams[0].users < 0).any()
    assert any(s.col_map is not None and (s.col_map < 0).any() for s in p.streams)
    assert (p.q_users < 0).any() and (p.q_users >= p.n_users).any() and np.unique(p.q_users).size < p.q_users.size
    assert (np.diff(p.extra_rp) == 0).any() and (np.diff(p.extra_rp) > 0).any()
    s0 = p.streams[0]
    for cap in (5, 64, 100):
        cut_in_a_run = short = only_missing = False
        for ev in dev.by_user[0]:
            if ev.size > cap:
                cut_in_a_run |= s0.times[ev[cap - 1]] == s0.times[ev[cap]]         # the cap falls between two events of equal time
                w = s0.items[ev[:cap]]
                short |= np.unique(w[w >= 0]).size < cap
                only_missing |= (w < 0).all()
        assert cut_in_a_run and short, cap
        assert only_missing or cap > 5, cap
    # a user in each class with n_u above and below the cap: caps 5 and 5000 against 63 / 4095 / 10000 events; 100 against 65 and 64
    n_u = np.array([r.size for r in dev.by_user[0]])
    for lo, hi in ((1, 64), (65, 4096), (4097, 1 << 30)):
        assert ((n_u >= lo) & (n_u <= hi) & (n_u > 5)).any() and ((n_u >= lo) & (n_u <= hi) & (n_u <= 5000)).any()
    # the history's exclusions overlap the extra rows
    _, want_excl = H.rows_ref(p, [5] * 3, dev.by_user, use_extra=False)
    assert any(np.intersect1d(want_excl[q], p.extra_ci[p.extra_rp[q]:p.extra_rp[q + 1]]).size for q in range(p.q_users.size))


def test_rows_do_not_depend_on_the_order_inside_the_index(sim_session, problem, dev):
    other = H.DeviceProblem(sim_session, problem, shuffle_index_seed=3)
    assert any(not torch.equal(a[2], b[2]) for a, b in zip(dev.ev, other.ev)), "the permuted index equals the built one"
    for cap in (5, 100):
        _, terms_a, excl_a = H.check(dev, [cap] * 3)
        _, terms_b, excl_b = H.check(other, [cap] * 3)
        for ra, rb in zip(terms_a + [excl_a], terms_b + [excl_b]):
            assert all(np.array_equal(x, y) for x, y in zip(ra, rb))


def test_bad_arguments(dev):
    s = dev.sess
    lib = s.lib
    nq = dev.q_users.numel()

    def call(events=None, n_types=None, extra=(None, None), rows=False, term_capacity=0, excl_capacity=0):
        events = events if events is not None else dev.events([5] * 3)
        arr = (_lib.HistEvent * max(len(events), 17))()
        keep = []
        for t, (n_cols, cap, bl, irp, ipos, items, times, cmap) in enumerate(events):
            rp, ci = s.empty(nq + 1, torch.int64), s.empty(8, torch.int32)
            keep += [rp, ci]
            arr[t].n_cols, arr[t].max_items, arr[t].blacklist = n_cols, cap, int(bl)
            arr[t].idx_row_ptr, arr[t].idx_pos, arr[t].items = irp.data_ptr(), ipos.data_ptr(), items.data_ptr() if items is not None else None
            arr[t].term_row_ptr, arr[t].term_col_idx, arr[t].term_capacity = rp.data_ptr(), ci.data_ptr(), term_capacity
        xrp = s.empty(nq + 1, torch.int64)
        n = len(events) if n_types is None else n_types
        if rows:
            return lib.urcco_dev_history_rows(s.handle, nq, dev.q_users.data_ptr(), dev.p.n_users, arr, n, extra[0], extra[1], dev.p.n_items, xrp.data_ptr(),
                                              xrp.data_ptr(), excl_capacity, None)
        return lib.urcco_dev_history_bounds(s.handle, nq, dev.q_users.data_ptr(), dev.p.n_users, arr, n, extra[0], extra[1], xrp.data_ptr())

    ok = dev.events([5] * 3)
    assert call() == _lib.OK
    for rows in (False, True):
        assert call(n_types=0, rows=rows) == _lib.BAD_ARG
        assert call(events=[ok[t % 3] for t in range(17)], rows=rows) == _lib.BAD_ARG
        assert call(events=[ok[0][:1] + (0,) + ok[0][2:]], rows=rows) == _lib.BAD_ARG                     # max_items < 1
        assert call(events=[ok[0][:5] + (None,) + ok[0][6:]], rows=rows) == _lib.BAD_ARG                   # a NULL the call needs
        assert call(extra=(dev.extra[0].data_ptr(), None), rows=rows) == _lib.BAD_ARG                      # a half-NULL extra pair
        assert call(extra=(None, dev.extra[1].data_ptr()), rows=rows) == _lib.BAD_ARG
    assert call(rows=True, term_capacity=-1) == _lib.BAD_ARG                                               # a negative capacity
    assert call(rows=True, excl_capacity=-1) == _lib.BAD_ARG
    assert call(events=ok[:2] + [ok[2]], rows=True, excl_capacity=-(1 << 40)) == _lib.BAD_ARG
    out = s.empty(4, torch.int64)
    assert lib.urcco_dev_history_index(s.handle, 1 << 31, out.data_ptr(), 1, out.data_ptr(), out.data_ptr()) == _lib.BAD_ARG   # n_events >= 2^31
    assert lib.urcco_dev_history_index(s.handle, 1, None, 1, out.data_ptr(), out.data_ptr()) == _lib.BAD_ARG
    assert lib.urcco_version() == 305


def test_no_queries_and_no_users(sim_session):
    p = H.Problem(0, 4, [H.Stream(4, np.zeros(0, np.int32), np.zeros(0, np.int32), None, None, True)], np.array([0, -1], np.int32), np.zeros(3, np.int64), np.zeros(0, np.int32))
    H.check(H.DeviceProblem(sim_session, p), [3])
    p.q_users = np.zeros(0, np.int32)
    p.extra_rp = np.zeros(1, np.int64)
    d = H.DeviceProblem(sim_session, p)
    terms, excl, _ = sim_session.history_rows(d.q_users[:0], 0, d.events([3]), 4, d.extra)   # no queries at all
    assert terms[0][0].tolist() == [0] and excl[0].tolist() == [0]


def test_restatement_orders_the_whole_int64_domain():
    """user_positions over INT64_MIN, -1, 0, INT64_MAX (duplicated: ties by position) against sorted() on Python ints; the subset form agrees"""
    rng = np.random.default_rng(1)
    special = [H.I64_MIN, -1, 0, H.I64_MAX, H.I64_MIN + 1, H.I64_MAX - 1, 1]
    times = np.array(special * 3 + [int(x) for x in rng.integers(-5, 5, 30)], np.int64)[rng.permutation(51)]
    users = rng.integers(-1, 3, 51).astype(np.int32)
    users[np.flatnonzero(np.isin(times, special[:4]))[::2]] = 1
    s = H.Stream(4, users, np.zeros(51, np.int32), times, None, True)
    got = H.user_positions(s, 3)
    sub = H.user_positions_of(s, [1, 2])
    for u in range(3):
        want = sorted((int(q) for q in np.flatnonzero(users == u)), key=lambda q: (int(times[q]), q), reverse=True)
        assert got[u].tolist() == want
        assert u == 0 or sub[u].tolist() == want
    assert {H.I64_MIN, -1, 0, H.I64_MAX} <= set(times[got[1]].tolist()) and sorted(sub) == [1, 2]
    s.times = None
    assert all(H.user_positions(s, 3)[u].tolist() == np.flatnonzero(users == u)[::-1].tolist() == H.user_positions_of(s, [u])[u].tolist() for u in range(3))


@pytest.fixture(scope="module")
def key_problem():
    return H.make_key_problem()


@pytest.fixture(scope="module")
def key_dev(sim_session, key_problem):
    return H.DeviceProblem(sim_session, key_problem)


def test_key_problem_holds_the_edge_cases(key_problem):
    H.assert_key_edge_cases(key_problem)


@pytest.mark.parametrize("cap", H.KEY_CAPS)
def test_key_domain_rows_match_the_restatement(key_dev, cap):
    stats, _, _ = H.check(key_dev, [cap, cap])
    assert stats[0] > 0 and stats[1] > 0 and stats[2] > 0 and stats[3] > 0, stats


def test_key_domain_rows_do_not_depend_on_the_index_order_or_the_job_before(sim_session, key_problem, key_dev):
    other = H.DeviceProblem(sim_session, key_problem, shuffle_index_seed=4)
    assert not torch.equal(key_dev.ev[0][2], other.ev[0][2]), "the permuted index equals the built one"
    byte0 = H.DeviceProblem(sim_session, H.make_byte0_job())
    for cap in (20, 150, 2048):
        _, terms_a, excl_a = H.check(key_dev, [cap, 7])
        stats, _, _ = H.check(byte0, [100])           # one job whose keys differ in the lowest time byte alone, between two runs over every byte
        assert stats[1] == 1 and stats[3] == 1 and stats[0] + stats[2] == 0, stats
        _, terms_b, excl_b = H.check(other, [cap, 7])
        for ra, rb in zip(terms_a + [excl_a], terms_b + [excl_b]):
            assert all(np.array_equal(x, y) for x, y in zip(ra, rb))


def test_positions_beyond_2_24(sim_session):
    """The most significant position digit differs and decides (no times / equal times); caps below, at and above each user's number of events at or
    above 2^24.  The index of the five users is built on the host: the simulator does not run the index kernels over 17 M events."""
    p = H.make_far_problem()
    d = H.DeviceProblem(sim_session, p, subset=range(p.n_users), host_index=True)
    for cap in H.far_caps(p):
        stats, terms, _ = H.check(d, [cap, cap])
        assert stats[0] > 0 and stats[1] > 0 and stats[2] > 0 and stats[3] > 0, stats
        assert np.array_equal(terms[0][3], terms[1][3])          # without times and with equal times: the same window


@pytest.mark.parametrize("cap", (5, 100))
def test_capacity_below_the_bounds(dev, cap):
    """Buffers of exactly max(capacity, 1) entries: under HIPSIM_GUARD a write past them faults."""
    H.capacity_cases(dev, [cap] * 3)


def test_under_guard_pages():
    """This module once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument)."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    env = dict(os.environ, HIPSIM_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
