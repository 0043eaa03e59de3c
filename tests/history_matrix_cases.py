"""urcco_dev_history_users / urcco_dev_history_matrix (decision D23 of DESIGN.md, include/urcco.h): the problems and checks that
tests/test_sim_history_matrix.py and tests/test_gpu_history_matrix.py share.  The contract, restated in numpy (users_ref, matrix_ref):

    w[p]       = times is None or (t_lo <= times[p] and (t_hi == INT64_MAX or times[p] < t_hi))
    c[u]       = the number of index entries e of user u with w[pos[e]];  keep[u] = c[u] >= min_events
    row_of[u]  = the number of kept users below u if keep[u] else -1;  n_rows = keep.sum()
    row r      = sorted distinct items[pos[e]] in 0 .. n_cols over the entries e with w[pos[e]] of the user u with row_of[u] == r (identity without
                 row_of), provided 0 <= r < n_rows and row_ptr[u + 1] <= capacity; every other row is empty

Every index here is built on the host, in a random order inside every user's segment, and holds exactly n_e entries: a read past them faults under
HIPSIM_GUARD.  run_matrix allocates out_row_ptr at exactly n_rows + 1 and out_col_idx at exactly max(capacity, 1) entries plus `pad` sentinel entries
each, and check asserts that the padding still holds the sentinel."""
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import history_ref as H
import history_trim_cases as T
from history_append_cases import put
from universal_recommender_amd import _lib

I64_MIN, I64_MAX = H.I64_MIN, H.I64_MAX
I32_MAX = (1 << 31) - 1
SENTINEL = H.SENTINEL
T0 = T.T0
OPEN = (I64_MIN, I64_MAX)
WAVE, LDS = 64, 4096                      # the class limits: raw entries of a user one wave / one block in LDS takes
EDGE_COUNTS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 9000)
EDGE_COLS = (1, 31, 32, 33, 300, 257 * 32 + 1)      # bitmap word edges; the last: more than one round of 256 words in the walk


@dataclass
class MatProblem:
    name: str
    n_users: int
    n_cols: int
    items: np.ndarray             # int32 [n_events]
    times: Optional[np.ndarray]   # int64 [n_events] or None
    rp: np.ndarray                # int64 [n_users + 1]
    pos: np.ndarray               # int32 [n_e]

    @property
    def n_events(self):
        return int(self.items.size)


def from_users(name, users, n_users, n_cols, items, times, rng):
    rp, pos = T.host_index(users, n_users, rng)
    return MatProblem(name, n_users, n_cols, items.astype(np.int32), times, rp, pos)


def classes_of(rp):
    """users per class (wave, block, bitmap) by their raw entries, from the host copy of the index; users without entries are in none"""
    m = np.diff(rp)
    return int(((m > 0) & (m <= WAVE)).sum()), int(((m > WAVE) & (m <= LDS)).sum()), int((m > LDS).sum())


# ---- the contract in numpy ------------------------------------------------------------------------------------------------------------------------
def window_ref(times, n, t_lo, t_hi):
    if times is None:
        return np.ones(n, bool)
    return (times >= t_lo) & ((times < t_hi) | (t_hi == I64_MAX))


def users_ref(t: MatProblem, t_lo, t_hi, min_events):
    w = window_ref(t.times, t.n_events, t_lo, t_hi)
    user_of = np.repeat(np.arange(t.n_users), np.diff(t.rp))
    c = np.bincount(user_of[w[t.pos]], minlength=t.n_users)
    keep = c >= min_events
    row_of = np.where(keep, np.cumsum(keep) - keep, -1).astype(np.int32)
    return row_of, int(keep.sum()), c


def matrix_ref(t: MatProblem, t_lo, t_hi, row_of, n_rows, capacity):
    """(row_ptr int64 [n_rows + 1], col_idx int32 [nnz]) of a well-formed index and a row_of that names no row twice"""
    user_of = np.repeat(np.arange(t.n_users), np.diff(t.rp))
    r = (user_of if row_of is None else row_of[user_of]).astype(np.int64)
    it = t.items[t.pos].astype(np.int64)
    ok = (r >= 0) & (r < n_rows) & (t.rp[1:][user_of] <= capacity) & window_ref(t.times, t.n_events, t_lo, t_hi)[t.pos] & (it >= 0) & (it < t.n_cols)
    key = np.unique(r[ok] * t.n_cols + it[ok])
    rows, cols = key // t.n_cols, key % t.n_cols
    return np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_rows))]).astype(np.int64), cols.astype(np.int32)


# ---- the calls ------------------------------------------------------------------------------------------------------------------------------------
def _ptr(x):
    return x.data_ptr() if x is not None and x.numel() else None      # an array of no entries is passed as NULL


def _device(sess, t: MatProblem):
    """the problem's arrays in tensors of exactly their sizes; `times` of a timed stream without events is one placeholder entry (NULL means untimed)"""
    d_times = None if t.times is None else (put(sess, t.times) if t.n_events else sess.empty(1, torch.int64))
    d_pos = put(sess, t.pos) if t.pos.size or not t.n_events else sess.empty(1, torch.int32)     # an index without entries still has an array
    return put(sess, t.items), d_times, put(sess, t.rp), d_pos


def run_users(sess, t: MatProblem, t_lo, t_hi, min_events, pad=0):
    """One urcco_dev_history_users call through ctypes: (status, row_of [n_users + pad], n_rows)"""
    _, d_times, d_rp, d_pos = _device(sess, t)
    row_of = sess.empty(max(t.n_users, 1) + pad, torch.int32)
    row_of.fill_(SENTINEL)
    n_rows = sess.empty(1, torch.int64)
    n_rows.fill_(SENTINEL)
    status = sess.lib.urcco_dev_history_users(sess.handle, t.n_events, d_times.data_ptr() if d_times is not None else None, t.n_users, d_rp.data_ptr(), _ptr(d_pos),
                                              t_lo, t_hi, min_events, row_of.data_ptr(), n_rows.data_ptr())
    sess.synchronize()
    return status, row_of.cpu().numpy(), int(n_rows[0])


def run_matrix(sess, t: MatProblem, t_lo, t_hi, row_of, n_rows, capacity, pad=0):
    """One urcco_dev_history_matrix call through ctypes: (status, row_ptr [n_rows + 1 + pad], col_idx [max(capacity, 1) + pad], nnz)"""
    d_items, d_times, d_rp, d_pos = _device(sess, t)
    d_row_of = put(sess, np.asarray(row_of, np.int32)) if row_of is not None else None
    rp = sess.empty(n_rows + 1 + pad, torch.int64)
    ci = sess.empty(max(capacity, 1) + pad, torch.int32)
    nnz = sess.empty(1, torch.int64)
    for o in (rp, ci, nnz):
        o.fill_(SENTINEL)
    status = sess.lib.urcco_dev_history_matrix(sess.handle, t.n_events, _ptr(d_items), d_times.data_ptr() if d_times is not None else None, t.n_users, d_rp.data_ptr(),
                                               _ptr(d_pos), t_lo, t_hi, t.n_cols, d_row_of.data_ptr() if d_row_of is not None else None, n_rows, rp.data_ptr(),
                                               ci.data_ptr(), capacity, nnz.data_ptr())
    sess.synchronize()
    return status, rp.cpu().numpy(), ci.cpu().numpy(), int(nnz[0])


def check_matrix(sess, t: MatProblem, window, row_of, n_rows, capacity=None, pad=0):
    capacity = t.n_events if capacity is None else capacity
    w_rp, w_ci = matrix_ref(t, window[0], window[1], row_of, n_rows, capacity)
    status, rp, ci, nnz = run_matrix(sess, t, window[0], window[1], row_of, n_rows, capacity, pad)
    assert status == _lib.OK, t.name
    assert nnz == w_rp[-1] == w_ci.size, (t.name, nnz, int(w_rp[-1]))
    assert np.array_equal(rp[: n_rows + 1], w_rp), t.name
    assert np.array_equal(ci[:nnz], w_ci), t.name
    assert (rp[n_rows + 1:] == SENTINEL).all() and (ci[max(capacity, 1):] == SENTINEL).all(), f"{t.name}: written at or past out_row_ptr[n_rows + 1] / out_col_idx[capacity]"
    assert rp.size == n_rows + 1 + pad and ci.size == max(capacity, 1) + pad
    return w_rp, w_ci


def check(sess, t: MatProblem, window=OPEN, min_events=1, capacity=None, pad=0):
    """_users, then _matrix with its output, both against the restatement.  Returns (row_of, n_rows, row_ptr, col_idx) of the restatement."""
    w_row_of, w_n_rows, _ = users_ref(t, window[0], window[1], min_events)
    status, row_of, n_rows = run_users(sess, t, window[0], window[1], min_events, pad)
    assert status == _lib.OK, t.name
    assert n_rows == w_n_rows and np.array_equal(row_of[: t.n_users], w_row_of), (t.name, n_rows, w_n_rows)
    assert (row_of[max(t.n_users, 1):] == SENTINEL).all(), f"{t.name}: written at or past out_row_of[n_users]"
    w_rp, w_ci = check_matrix(sess, t, window, w_row_of, w_n_rows, capacity, pad)
    return w_row_of, w_n_rows, w_rp, w_ci


def rows_of(rp, ci):
    return [ci[rp[r]:rp[r + 1]] for r in range(rp.size - 1)]


# ---- class edges ----------------------------------------------------------------------------------------------------------------------------------
def make_edge_problem(n_cols, seed=3):
    """One stream: users of EDGE_COUNTS raw entries with random items in -1 .. n_cols (both ends outside the columns); per class (10, 100, 5000 entries) a
    user whose events all carry one column and one whose items are all outside the columns (-1, n_cols, INT32_MAX); a heavy user in whose row every column
    is set; empty users at both ends; some positions are nobody's.  Returns (problem, {name: user})."""
    rng = np.random.default_rng(seed + n_cols)
    full = max(n_cols, LDS + 1) + 7
    counts = [0] + list(EDGE_COUNTS) + [10, 100, 5000] + [10, 100, 5000] + [full, 0, 0]
    named = {"edge": 1, "one column": 1 + len(EDGE_COUNTS), "outside": 4 + len(EDGE_COUNTS), "full": 7 + len(EDGE_COUNTS)}
    n_users = len(counts)
    users = np.concatenate([np.repeat(np.arange(n_users, dtype=np.int32), counts), np.full(9, -1, np.int32)])
    items = rng.integers(-1, n_cols + 1, users.size).astype(np.int64)
    for k in range(3):
        items[users == named["one column"] + k] = n_cols - 1 if k else 0
        items[users == named["outside"] + k] = np.array([-1, n_cols, I32_MAX])[rng.integers(0, 3, counts[named["outside"] + k])]
    items[users == named["full"]] = np.arange(full) % n_cols
    order = rng.permutation(users.size)
    return from_users(f"edges n_cols={n_cols}", users[order], n_users, n_cols, items[order], None, rng), named


def edge_cases(sess):
    for n_cols in EDGE_COLS:
        t, named = make_edge_problem(n_cols)
        m = np.diff(t.rp)
        assert tuple(m[named["edge"]:named["edge"] + len(EDGE_COUNTS)]) == EDGE_COUNTS and min(classes_of(t.rp)) >= 3 and m[0] == 0 and m[-1] == 0
        row_of, n_rows, rp, ci = check(sess, t)
        rows = rows_of(rp, ci)
        assert n_rows == int((m > 0).sum())
        for k in range(3):       # all one column: one entry; only items outside the columns: a kept user with an empty row, the heavy one among them
            assert rows[row_of[named["one column"] + k]].tolist() == [n_cols - 1 if k else 0]
            assert row_of[named["outside"] + k] >= 0 and rows[row_of[named["outside"] + k]].size == 0
        assert np.array_equal(rows[row_of[named["full"]]], np.arange(n_cols))       # every column set
        if n_cols <= 300:
            assert np.array_equal(rows[row_of[named["edge"] + len(EDGE_COUNTS) - 1]], np.arange(n_cols))
    t, _ = make_edge_problem(33)
    check(sess, t, pad=70)                        # padded buffers: the padding is untouched
    check_matrix(sess, t, OPEN, None, t.n_users)      # row_of == NULL: every user is its own row
    for t in (MatProblem("no events", 4, 5, np.zeros(0, np.int32), None, np.zeros(5, np.int64), np.zeros(0, np.int32)),
              MatProblem("no users", 0, 5, np.arange(3, dtype=np.int32), None, np.zeros(1, np.int64), np.zeros(0, np.int32))):
        _, n_rows, rp, _ = check(sess, t)
        assert n_rows == 0 and rp.tolist() == [0]


# ---- the window -----------------------------------------------------------------------------------------------------------------------------------
TIME_VALUES = (I64_MIN, I64_MIN + 1, -(1 << 40), -1, 0, 1, T0 - 1, T0, T0 + 1, I64_MAX - 1, I64_MAX)
WINDOWS = (OPEN, (T0, T0), (T0, T0 + 1), (T0 - 1, T0 + 1), (0, I64_MAX), (I64_MIN, 0), (I64_MIN + 1, I64_MAX - 1), (I64_MAX, I64_MAX), (I64_MIN, I64_MIN),
           (I64_MAX - 1, I64_MAX), (1, -1), (T0 + 2, T0 + 5))


def make_window_problem(seed=7):
    """Times over the whole int64 domain; users of every class; a heavy user whose events all lie at T0 + 3 (inside the last window only)"""
    rng = np.random.default_rng(seed)
    counts = [0, 3, 64, 65, 700, 5000, 4500, 1, 0]
    n_users, n_cols = len(counts), 97
    users = np.repeat(np.arange(n_users, dtype=np.int32), counts)
    times = np.array(TIME_VALUES, np.int64)[rng.integers(0, len(TIME_VALUES), users.size)]
    times[users == 6] = T0 + 3
    times[users == 7] = T0
    order = rng.permutation(users.size)
    return from_users("window", users[order], n_users, n_cols, rng.integers(-1, n_cols + 1, users.size), times[order], rng)


def window_cases(sess):
    t = make_window_problem()
    assert min(classes_of(t.rp)) >= 2 and set(TIME_VALUES) <= set(t.times.tolist())
    seen = {}
    for win in WINDOWS:
        for min_events in (1, 2):
            row_of, n_rows, rp, ci = check(sess, t, win, min_events)
            seen[win, min_events] = (row_of, n_rows, int(rp[-1]))
    w = lambda win: window_ref(t.times, t.n_events, *win)      # noqa: E731
    assert w(OPEN).all() and not w((T0, T0)).any() and not w((1, -1)).any()                          # t_lo == t_hi: nothing
    assert np.array_equal(w((T0, T0 + 1)), t.times == T0)                                            # equality at the start: in; at the end: out
    assert np.array_equal(w((T0 - 1, T0 + 1)), (t.times == T0) | (t.times == T0 - 1))
    assert np.array_equal(w((I64_MAX, I64_MAX)), t.times == I64_MAX) and (t.times == I64_MAX).any()  # t_hi == INT64_MAX: open, events at INT64_MAX are in
    assert np.array_equal(w((I64_MAX - 1, I64_MAX)), t.times >= I64_MAX - 1)
    assert not w((I64_MIN + 1, I64_MAX - 1))[(t.times == I64_MIN) | (t.times >= I64_MAX - 1)].any()
    assert seen[(T0, T0), 1][1] == 0 and seen[(T0, T0), 1][2] == 0
    assert seen[(T0, T0 + 1), 1][0][7] >= 0 and seen[(T0, T0 + 1), 2][0][7] == -1                    # the user of one event at T0
    assert seen[(T0 + 2, T0 + 5), 1][0][6] == 0 and seen[(T0, T0 + 1), 1][0][6] == -1                # the heavy user is the only one / has no event in the window
    # an untimed stream: the open window only
    u = MatProblem("untimed", t.n_users, t.n_cols, t.items, None, t.rp, t.pos)
    check(sess, u)
    for win in ((T0, I64_MAX), (I64_MIN, T0), (T0, T0)):
        assert run_users(sess, u, win[0], win[1], 1)[0] == _lib.BAD_ARG
        assert run_matrix(sess, u, win[0], win[1], None, u.n_users, u.n_events)[0] == _lib.BAD_ARG


# ---- users ----------------------------------------------------------------------------------------------------------------------------------------
def make_user_problems(seed=11):
    """A primary and a secondary stream over 14 users.  Primary: user 2 has 5 events of which 4 lie outside the window, user 3's events all do, user 4
    has 5 events that all carry items < 0, user 5 has 2 events, user 6 one, user 7 a heavy row, users 0, 1, 12, 13 nothing.  Secondary: every user has
    events, also those the primary drops."""
    rng = np.random.default_rng(seed)
    counts = [0, 0, 5, 6, 5, 2, 1, 4200, 70, 64, 9, 5, 0, 0]
    n_users, n_cols = len(counts), 40
    users = np.repeat(np.arange(n_users, dtype=np.int32), counts)
    times = (T0 + rng.integers(0, 50, users.size)).astype(np.int64)
    times[users == 3] = T0 - 5
    times[np.flatnonzero(users == 2)[:4]] = T0 + 100
    items = rng.integers(0, n_cols, users.size)
    items[users == 4] = -1
    order = rng.permutation(users.size)
    prim = from_users("primary", users[order], n_users, n_cols, items[order], times[order], rng)
    counts2 = rng.integers(1, 90, n_users)
    counts2[3] = 4300
    users2 = np.repeat(np.arange(n_users, dtype=np.int32), counts2)
    users2 = users2[rng.permutation(users2.size)]
    sec = from_users("secondary", users2, n_users, 300, rng.integers(-1, 301, users2.size), (T0 + rng.integers(-20, 70, users2.size)).astype(np.int64), rng)
    return prim, sec


def user_cases(sess):
    prim, sec = make_user_problems()
    win = (T0, T0 + 50)
    for min_events in (1, 2, 5):
        row_of, n_rows, rp, ci = check(sess, prim, win, min_events)
        _, _, c = users_ref(prim, win[0], win[1], min_events)
        assert c[2] == 1 and c[3] == 0 and c[4] == 5 and c[5] == 2 and c[6] == 1
        assert row_of[3] == -1 and (row_of[2] >= 0) == (min_events == 1) and (row_of[5] >= 0) == (min_events <= 2) and (row_of[6] >= 0) == (min_events == 1)
        assert row_of[4] >= 0 and rp[row_of[4] + 1] == rp[row_of[4]]       # kept through events without a column: an empty row
        assert row_of[7] >= 0 and row_of[0] == row_of[13] == -1
        # the secondary keeps the events of the primary's users only: its heavy user 3 is dropped
        s_rp, s_ci = check_matrix(sess, sec, win, row_of, n_rows)
        assert s_rp.size == n_rows + 1 and 0 < s_rp[-1] < sec.n_events
        want = matrix_ref(sec, win[0], win[1], None, sec.n_users, sec.n_events)
        assert np.array_equal(np.concatenate(rows_of(s_rp, s_ci)), np.concatenate([r for u, r in enumerate(rows_of(*want)) if row_of[u] >= 0]))
    # row_of == NULL, and a row_of whose entries reach past n_rows: those users are ignored
    check_matrix(sess, prim, win, None, prim.n_users)
    check_matrix(sess, sec, OPEN, None, sec.n_users)
    row_of, n_rows, _ = users_ref(prim, win[0], win[1], 1)
    assert n_rows >= 6
    rp3, _ = check_matrix(sess, sec, win, row_of, 3, pad=5)
    assert rp3.size == 4 and rp3[-1] > 0
    assert run_matrix(sess, sec, win[0], win[1], None, sec.n_users - 1, sec.n_events)[0] == _lib.BAD_ARG       # identity needs n_rows == n_users


# ---- several heavy rows per block -----------------------------------------------------------------------------------------------------------------
def heavy_rows_case(sess):
    """URCCO_HM_BITMAP_BUDGET=0 leaves the bitmap class one block: it serves every heavy row in turn, in whatever order the list holds them.  Every
    heavy user's columns are a band of its own, so a bit that survived a row shows up as a wrong column in every later row."""
    rng = np.random.default_rng(29)
    n_heavy, n_cols = 7, 257 * 32 + 1
    counts = [LDS + 1 + 13 * k for k in range(n_heavy)] + [30, 0, 200]
    n_users = len(counts)
    users = np.repeat(np.arange(n_users, dtype=np.int32), counts)
    band = n_cols // n_heavy
    items = rng.integers(0, n_cols, users.size)
    for k in range(n_heavy):
        items[users == k] = k * band + rng.integers(0, band, counts[k])
    items[users == 3] = -1      # a heavy row without a kept entry between the others
    order = rng.permutation(users.size)
    t = from_users("heavy rows", users[order], n_users, n_cols, items[order], None, rng)
    assert classes_of(t.rp)[2] == n_heavy
    old = os.environ.get("URCCO_HM_BITMAP_BUDGET")
    try:
        for budget in ("0", None):
            if budget is None:
                os.environ.pop("URCCO_HM_BITMAP_BUDGET", None)
            else:
                os.environ["URCCO_HM_BITMAP_BUDGET"] = budget
            row_of, _, rp, ci = check(sess, t)
            rows = rows_of(rp, ci)
            assert rows[row_of[3]].size == 0 and all(rows[row_of[k]].min() >= k * band and rows[row_of[k]].max() < (k + 1) * band for k in range(n_heavy) if k != 3)
    finally:
        if old is None:
            os.environ.pop("URCCO_HM_BITMAP_BUDGET", None)
        else:
            os.environ["URCCO_HM_BITMAP_BUDGET"] = old


# ---- capacity -------------------------------------------------------------------------------------------------------------------------------------
def capacity_cases(sess):
    """capacity == the bound total: every row; one less: the last user with entries loses its row, the rows before it are whole; in the middle of a
    heavy row; 0.  out_col_idx has exactly max(capacity, 1) entries, out_row_ptr exactly n_rows + 1."""
    t, _ = make_edge_problem(300)
    total = int(t.rp[-1])
    whole = check(sess, t, capacity=total)
    last = int(np.flatnonzero(np.diff(t.rp) > 0)[-1])
    heavy = int(np.flatnonzero(np.diff(t.rp) > LDS)[0])
    for cap in (total - 1, int(t.rp[heavy + 1]) - 1, int(t.rp[heavy + 1]), 1, 0):
        row_of, n_rows, rp, ci = check(sess, t, capacity=cap)
        fits = t.rp[1:] <= cap
        assert np.array_equal(row_of, whole[0]) and n_rows == whole[1]                # _users does not know the capacity
        for u in np.flatnonzero(row_of >= 0):
            got, want = ci[rp[row_of[u]]:rp[row_of[u] + 1]], whole[3][whole[2][row_of[u]]:whole[2][row_of[u] + 1]]
            assert np.array_equal(got, want) if fits[u] else got.size == 0, (cap, u)
        assert rp[-1] <= cap
        if cap == total - 1:
            assert not fits[last] and fits[:last].all() and whole[2][row_of[last] + 1] > whole[2][row_of[last]]


# ---- a hostile index ------------------------------------------------------------------------------------------------------------------------------
def hostile_cases(sess):
    """Whatever idx_row_ptr, idx_pos and row_of hold: URCCO_OK, the run ends, no access leaves the arrays (HIPSIM_GUARD).  The stream and the index
    generators are those of history_trim_cases: make_user_problem (a user of 5000 entries, users of 63 / 64 / 65, runs of empty ones) and host_index.  idx_pos
    holds n_events entries, the capacity urcco_dev_history_index states: the clamp of the row starts promises no more."""
    rng = np.random.default_rng(19)
    base, _ = T.make_user_problem(big=5000)
    n, n_users = base.n_events, base.n_users
    rp = base.row_ptr
    pos = np.concatenate([base.pos, rng.integers(0, n, n - base.pos.size).astype(np.int32)])      # n_events entries: a row_ptr that lies may claim up to that many
    bad_pos = pos.copy()
    bad_pos[rng.permutation(pos.size)[:300]] = np.array([-1, n, I32_MAX, -(1 << 31)], np.int32)[rng.integers(0, 4, 300)]
    bad_pos[[0, 63, 64, pos.size - 1]] = (-1, n, I32_MAX, n)
    descending = rp[::-1].copy()
    beyond = rp + np.arange(n_users + 1) * 400
    jumpy = rp.copy()
    jumpy[[2, 5, 7]] = (-50, 1 << 40, I64_MIN)
    overlap = np.where(np.arange(n_users + 1) % 2 == 0, 0, pos.size).astype(np.int64)      # every other user owns the whole index: the raw rows sum to many times n_e
    n_rows = 7
    row_ofs = {"null": None, "kept": users_ref(MatProblem("", n_users, 50, base.items, base.times, rp, base.pos), *OPEN, 1)[0],
               "hostile": np.array([0, 0, -1, n_rows, I32_MAX, -(1 << 31), 6, 5, 5, 4, 3, 3, 2, 1, 0, 6, 6, 0], np.int32)[:n_users]}
    assert row_ofs["hostile"].size == n_users
    for name, h_rp, h_pos in (("pos", rp, bad_pos), ("descending", descending, pos), ("beyond", beyond, pos), ("jumpy", jumpy, bad_pos), ("both", beyond[::-1].copy(), bad_pos),
                              ("overlap", overlap, pos), ("overlap, bad pos", overlap, bad_pos)):
        for times in (base.times, None):
            t = MatProblem(f"hostile {name}", n_users, 50, base.items, times, h_rp, h_pos)
            win = (T0, T0 + 10) if times is not None else OPEN
            status, row_of, k = run_users(sess, t, win[0], win[1], 2)
            assert status == _lib.OK and 0 <= k <= n_users and ((row_of[:n_users] >= -1) & (row_of[:n_users] < max(k, 1))).all(), (name, k)
            for rname, r in row_ofs.items():
                nr = n_users if r is None else (n_rows if rname == "hostile" else int(r.max()) + 1)
                for cap in (n, 100, 0):
                    status, o_rp, o_ci, nnz = run_matrix(sess, t, win[0], win[1], r, nr, cap, pad=3)
                    assert status == _lib.OK and nnz >= 0 and (o_rp[nr + 1:] == SENTINEL).all() and (o_ci[max(cap, 1):] == SENTINEL).all(), (name, rname, cap)


# ---- against urcco_dev_csr_from_pairs -------------------------------------------------------------------------------------------------------------
def pairs_problems():
    """Three random streams with their users: the two of history_ref.make_stream_history (a timed one with ids outside the dictionary, an untimed one)
    and one of the same form with a Zipf user distribution whose head owns more than 4096 events"""
    streams, _ = H.make_stream_history(53, 120, 90, 60)
    out = [(ev, u, i, t, 90 if ev == "purchase" else 60, 120) for ev, (u, i, t) in streams.items()]
    rng = np.random.default_rng(59)
    n, n_users = 30000, 500
    users = ((rng.zipf(1.3, n) - 1) % n_users).astype(np.int32)
    users[rng.integers(0, n, 40)] = -1
    assert np.bincount(users[users >= 0]).max() > LDS
    out.append(("zipf", users, rng.integers(-1, 2000, n).astype(np.int32), (T0 + rng.integers(-500, 500, n)).astype(np.int64), 1999, n_users))
    return out


def pairs_cases(sess):
    """_users + _matrix over the device-built index == urcco_dev_csr_from_pairs over the filtered, renumbered pairs: row_ptr, col_idx[:nnz], nnz bit for bit"""
    from universal_recommender_amd.ingest import csr_from_pairs
    for name, users, items, times, n_cols, n_users in pairs_problems():
        n = users.size
        d_users, d_items, d_times = put(sess, users), put(sess, items), put(sess, times) if times is not None else None
        rp, pos = sess.history_index(d_users, n_users)
        for after, before, min_events in ((None, None, 1), (None, None, 3)) + (((int(np.median(times)), None, 2), (int(np.quantile(times, 0.2)), int(np.quantile(times, 0.8)), 1))
                                                                                if times is not None else ()):
            row_of, n_rows = sess.history_users(n, d_times, rp, pos[:n], after, before, min_events)
            k = int(n_rows[0])
            o_rp, o_ci, o_nnz = sess.history_matrix(n, d_items, d_times, rp, pos[:n], n_cols, row_of, k, after, before)
            sess.synchronize()
            w = window_ref(times, n, I64_MIN if after is None else after, I64_MAX if before is None else before)
            h_row_of = row_of.cpu().numpy()
            ok = w & (users >= 0) & (items >= 0) & (items < n_cols)
            ok[ok] = h_row_of[users[ok]] >= 0
            m = csr_from_pairs(sess, put(sess, h_row_of[users[ok]]), put(sess, items[ok]), k, n_cols)
            sess.synchronize()
            nnz = int(o_nnz[0])
            assert 0 < k <= n_users and 0 < nnz == m.nnz_bound, (name, k, nnz, m.nnz_bound)
            assert torch.equal(o_rp[: k + 1].cpu(), m.row_ptr[: k + 1].cpu()) and torch.equal(o_ci[:nnz].cpu(), m.col_idx[:nnz].cpu()), name


# ---- bad arguments --------------------------------------------------------------------------------------------------------------------------------
def bad_argument_cases(sess):
    lib = sess.lib
    t = make_window_problem()
    n, nu = t.n_events, t.n_users
    d = dict(items=put(sess, t.items), times=put(sess, t.times), rp=put(sess, t.rp), pos=put(sess, t.pos), row_of=put(sess, np.arange(nu, dtype=np.int32)),
             o_row_of=sess.empty(nu, torch.int32), o_n=sess.empty(1, torch.int64), o_rp=sess.empty(nu + 1, torch.int64), o_ci=sess.empty(n, torch.int32),
             o_nnz=sess.empty(1, torch.int64))
    ok = dict(s=sess.handle, n=n, nu=nu, lo=T0, hi=I64_MAX, min_events=1, n_cols=t.n_cols, n_rows=nu, cap=n, **{k: v.data_ptr() for k, v in d.items()})

    def users(**kw):
        a = dict(ok, **kw)
        return lib.urcco_dev_history_users(a["s"], a["n"], a["times"], a["nu"], a["rp"], a["pos"], a["lo"], a["hi"], a["min_events"], a["o_row_of"], a["o_n"])

    def matrix(**kw):
        a = dict(ok, **kw)
        return lib.urcco_dev_history_matrix(a["s"], a["n"], a["items"], a["times"], a["nu"], a["rp"], a["pos"], a["lo"], a["hi"], a["n_cols"], a["row_of"], a["n_rows"],
                                            a["o_rp"], a["o_ci"], a["cap"], a["o_nnz"])

    assert users() == _lib.OK and matrix() == _lib.OK
    for call in (users, matrix):
        assert call(n=1 << 31) == _lib.BAD_ARG and call(n=1 << 62) == _lib.BAD_ARG      # n_events >= 2^31
        assert call(n=-1) == _lib.BAD_ARG and call(nu=-1) == _lib.BAD_ARG and call(nu=0x7ffffff1) == _lib.BAD_ARG
        assert call(times=None) == _lib.BAD_ARG and call(times=None, lo=I64_MIN, hi=T0) == _lib.BAD_ARG and call(times=None, lo=I64_MIN + 1) == _lib.BAD_ARG
        assert call(times=None, lo=I64_MIN, hi=I64_MAX) == _lib.OK
        for name in ("s", "rp", "pos"):
            assert call(**{name: None}) == _lib.BAD_ARG, name
    assert users(min_events=0) == _lib.BAD_ARG and users(min_events=-3) == _lib.BAD_ARG
    assert users(o_row_of=None) == _lib.BAD_ARG and users(o_n=None) == _lib.BAD_ARG
    assert matrix(n_cols=0) == _lib.BAD_ARG and matrix(n_cols=-1) == _lib.BAD_ARG and matrix(n_rows=-1) == _lib.BAD_ARG and matrix(cap=-1) == _lib.BAD_ARG
    assert matrix(row_of=None, n_rows=nu - 1) == _lib.BAD_ARG and matrix(row_of=None) == _lib.OK
    for name in ("items", "o_rp", "o_ci", "o_nnz"):
        assert matrix(**{name: None}) == _lib.BAD_ARG, name
    # NULLs the calls do not need
    assert matrix(cap=0, o_ci=None) == _lib.OK
    assert users(n=0, pos=None) == _lib.OK and matrix(n=0, items=None, pos=None) == _lib.OK
    assert users(nu=0, rp=None, o_row_of=None) == _lib.OK and matrix(nu=0, rp=None, row_of=None, n_rows=0) == _lib.OK
    sess.synchronize()
    assert int(d["o_n"][0]) == 0 and int(d["o_rp"][0]) == 0 and int(d["o_nnz"][0]) == 0
    assert lib.urcco_version() == 305


# ---- DeviceHistory.matrices and URAlgorithm.train_from_history ------------------------------------------------------------------------------------
def device_streams(sess, streams, lo=None, hi=None):
    return {ev: tuple(torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(sess.device) if a is not None else None for a in st) for ev, st in streams.items()}


def timed_streams(seed, n_users, n_items, n_view):
    """history_ref.make_stream_history with times on the "view" stream as well: a window can apply to every type"""
    streams, _ = H.make_stream_history(seed, n_users, n_items, n_view)
    t = streams["purchase"][2]
    u, i, _ = streams["view"]
    streams["view"] = (u, i, np.random.default_rng(seed).choice(t, u.size))
    return streams


def pairs_matrices(sess, streams, events, n_users, n_cols, after_ms, before_ms, min_events):
    """The other route to DeviceHistory.matrices, from the streams' `users` arrays: the window, the users with at least min_events primary events in it
    renumbered in ascending id, csr_from_pairs per event type.  Returns (row_of, n_rows, {event: DevCsr})."""
    from universal_recommender_amd.ingest import csr_from_pairs
    win = {ev: window_ref(streams[ev][2], streams[ev][0].size, I64_MIN if after_ms is None else after_ms, I64_MAX if before_ms is None else before_ms) for ev in events}
    u0 = streams[events[0]][0]
    keep = np.bincount(u0[win[events[0]] & (u0 >= 0)], minlength=n_users) >= min_events
    row_of = np.where(keep, np.cumsum(keep) - keep, -1).astype(np.int32)
    n_rows = int(keep.sum())
    mats = {}
    for ev in events:
        u, i, _ = streams[ev]
        ok = win[ev] & (u >= 0) & (i >= 0) & (i < n_cols[ev])
        ok[ok] = row_of[u[ok]] >= 0
        mats[ev] = csr_from_pairs(sess, put(sess, row_of[u[ok]]), put(sess, i[ok]), n_rows, n_cols[ev])
    return row_of, n_rows, mats


def same_csr(a, b):
    nnz = int(a.row_ptr[-1])
    return (a.n_rows == b.n_rows and a.n_cols == b.n_cols and a.nnz_bound == b.nnz_bound == nnz and torch.equal(a.row_ptr.cpu(), b.row_ptr.cpu())
            and torch.equal(a.col_idx[:nnz].cpu(), b.col_idx[:nnz].cpu()))


def same_indicators(a, b):
    """two DevIndicators: row_ptr, col_idx and the LLR bits"""
    ra, ca, la = a.to_host()
    rb, cb, lb = b.to_host()
    return np.array_equal(ra, rb) and np.array_equal(ca, cb) and np.array_equal(la.view(np.int64), lb.view(np.int64))


def same_model(a, b):
    """two DeviceModels: the indicator matrices' CSR and the column starts of their CSC (the order inside a CSC column is the transposition's own and
    not specified)"""
    return a.n_items == b.n_items and len(a.correlators) == len(b.correlators) and all(
        x.name == y.name and x.n_cols == y.n_cols and torch.equal(x.row_ptr.cpu(), y.row_ptr.cpu()) and torch.equal(x.col_ptr.cpu(), y.col_ptr.cpu())
        and torch.equal(x.col_idx[: int(x.row_ptr[-1])].cpu(), y.col_idx[: int(y.row_ptr[-1])].cpu()) for x, y in zip(a.correlators, b.correlators))


def check_train_from_history(sess, n_model_rows, n_items, n_view, n_users, seed=47):
    """A history loaded in two parts (from_streams, append) and trimmed, retrained in a window with minEventsPerUser 3: (1) the indicator matrices of
    cross_occurrence_device over DeviceHistory.matrices are those over csr_from_pairs of the same events -- row_ptr, col_idx, LLR bits; (2) the model
    train_from_history returns is the one from_indicators builds from that route, and batch_predict over the two agrees."""
    from universal_recommender_amd.device import cross_occurrence_device
    from universal_recommender_amd.history import DeviceHistory
    from universal_recommender_amd.recommend import DeviceModel
    algo, model = H.predict_stack(sess, n_model_rows, n_items, n_view)
    algo.ap.seed, algo.ap.minEventsPerUser = 11, 3
    streams = timed_streams(seed, n_users, n_items, n_view)
    events, n_cols = ["purchase", "view"], {"purchase": n_items, "view": n_view}
    at = {ev: st[0].size * 2 // 3 for ev, st in streams.items()}
    dh = DeviceHistory.from_streams(sess, model, {ev: tuple(a[: at[ev]] for a in st) for ev, st in device_streams(sess, streams).items()}, n_users=n_users)
    dh.append({ev: tuple(a[at[ev]:] for a in st) for ev, st in device_streams(sess, streams).items()})
    t = np.sort(streams["purchase"][2])
    cut, drop = int(t[t.size // 10]), [3, 10, 41]
    dh.trim(before_ms=cut, drop_users=drop)
    left = {}
    for ev, (u, i, tm) in streams.items():
        keep = ~np.isin(u, drop) & (tm >= cut)
        left[ev] = (u[keep], i[keep], tm[keep])
    after, before = int(t[t.size // 4]), int(t[t.size * 9 // 10])
    w_row_of, w_n_rows, w_mats = pairs_matrices(sess, left, events, n_users, n_cols, after, before, 3)
    row_of, n_rows, mats = dh.matrices(events, after, before, 3)
    assert 0 < n_rows == w_n_rows < n_users and np.array_equal(row_of.cpu().numpy(), w_row_of) and all(same_csr(mats[ev], w_mats[ev]) for ev in events)
    params = algo._dataset_params(2)
    got = cross_occurrence_device(sess, [mats[ev] for ev in events], params, 11)
    want = cross_occurrence_device(sess, [w_mats[ev] for ev in events], params, 11)
    sess.synchronize()
    assert all(same_indicators(g, w) for g, w in zip(got, want)) and all(int(w.row_ptr[-1]) > 0 for w in want)
    new = algo.train_from_history(dh, after, before)
    ref = DeviceModel.from_indicators(sess, list(zip(events, want)), properties={})
    assert same_model(new, ref) and dh.model is model and not same_model(new, model)
    qs = [{"user": u} for u in range(0, n_users, 3)] + [{"user": u, "item": int(u * 2) % n_items} for u in range(1, n_users, 7)] + [{"user": n_users + 9}, {}, {"item": 5}]
    res = algo.batch_predict(ref, qs, dh)
    assert algo.batch_predict(new, qs, dh) == res and any(s["score"] > 0 for r in res for s in r["itemScores"])
    return algo, model, dh, left, (after, before)
