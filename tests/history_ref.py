"""Numpy restatement of decision D17 (include/urcco.h urcco_dev_history_*): the user-history term rows and the exclusion rows of a batch
of queries from event streams.  Written from the decision text, not from the kernels; the yardstick of tests/test_sim_history.py and
tests/test_gpu_history.py (the reference itself reads these from an event store behind a JVM).

    events of u     stream positions p with users[p] == u (users[p] < 0: nobody's)
    recency         (times[p] desc, p desc); without times the stream order is the time order
    window          the first min(n_u, cap) events in that order -- events with items[p] < 0 count toward the cap and give no column
    term row        the distinct items of the window, ascending
    exclusion row   union over the blacklist types of col_map[items[p]] over ALL events of u, entries < 0 dropped, united with the extra row; ascending
    unknown user    empty term rows, the exclusion row is the extra row alone
"""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

PLANTED = (0, 1, 63, 64, 65, 4095, 4096, 4097)   # both sides of the wave / block and the block / global boundary
HEAVY = 10000
CAPS = (1, 5, 64, 100, 5000)


@dataclass
class Stream:
    n_cols: int
    users: np.ndarray             # int32
    items: np.ndarray             # int32, < 0 = outside the column dictionary
    times: Optional[np.ndarray]   # int64 or None
    col_map: Optional[np.ndarray]  # int32 [n_cols] -> primary item id or -1; None = identity
    blacklist: bool


@dataclass
class Problem:
    n_users: int
    n_items: int
    streams: List[Stream]
    q_users: np.ndarray           # int32
    extra_rp: np.ndarray          # int64 [n_queries + 1]
    extra_ci: np.ndarray          # int32


def user_positions(s: Stream, n_users: int):
    """per user: the stream positions of its events, most recent first"""
    pos = np.arange(s.users.size, dtype=np.int64)
    t = s.times if s.times is not None else np.zeros(s.users.size, np.int64)
    order = np.lexsort((-pos, -t, s.users))            # by user, then time desc, then position desc
    order = order[s.users[order] >= 0]
    u = s.users[order]
    start = np.searchsorted(u, np.arange(n_users + 1))
    return [order[start[i]:start[i + 1]] for i in range(n_users)]


def rows_ref(p: Problem, caps, by_user=None, use_extra=True, blacklist=None):
    """(terms, excl): terms[t][q] and excl[q] as sorted unique int arrays"""
    by_user = by_user if by_user is not None else [user_positions(s, p.n_users) for s in p.streams]
    blacklist = blacklist if blacklist is not None else [s.blacklist for s in p.streams]
    none = np.zeros(0, np.int64)
    terms = [[] for _ in p.streams]
    excl = []
    for q, u in enumerate(p.q_users):
        known = 0 <= u < p.n_users
        x = [p.extra_ci[p.extra_rp[q]:p.extra_rp[q + 1]].astype(np.int64)] if use_extra else []
        for t, s in enumerate(p.streams):
            ev = by_user[t][u] if known else none
            window = s.items[ev[: min(ev.size, caps[t])]]
            terms[t].append(np.unique(window[window >= 0]))
            if blacklist[t]:
                it = s.items[ev]
                it = it[it >= 0]
                if s.col_map is not None:
                    it = s.col_map[it]
                x.append(it[it >= 0].astype(np.int64))
        excl.append(np.unique(np.concatenate(x)) if x else none)
    return terms, excl


def make_problem(seed=5, n_users=300, cols=(40, 500, 7), heavy=HEAVY, planted=PLANTED, time_values=50):
    """Three event types; type 0 is the primary (its columns are the items).  Planted per-type event counts per user on both sides of every class
    boundary and one heavy user; times from `time_values` values (ties are the rule), type 1 without times; 15 % of the events outside the column
    dictionary, a few events of nobody; column maps with -1 entries; queries: every user, unknown ones, repeats."""
    rng = np.random.default_rng(seed)
    n_items = cols[0]
    streams = []
    for t, n_cols in enumerate(cols):
        counts = rng.integers(0, 31, n_users)
        plant = list(planted) + ([heavy] if t == 0 else [])
        if t == 2:
            plant = [c for c in plant if c <= 65]
        who = rng.permutation(n_users)[: len(plant)]
        counts[who] = plant
        users = np.repeat(np.arange(n_users, dtype=np.int32), counts)
        users = np.concatenate([users, np.full(7, -1, np.int32)])
        users = users[rng.permutation(users.size)]
        items = rng.integers(0, n_cols, users.size).astype(np.int32)
        items[rng.random(users.size) < 0.15] = -1
        times = None if t == 1 else (1_600_000_000_000 + rng.integers(0, time_values, users.size)).astype(np.int64)
        col_map = None
        if t > 0:
            col_map = rng.integers(0, n_items, n_cols).astype(np.int32)
            col_map[rng.random(n_cols) < 0.3] = -1
        streams.append(Stream(n_cols, users, items, times, col_map, t < 2))
    # a user of type 0 whose 5 most recent events all lie outside the dictionary: windows made only of items < 0
    s0 = streams[0]
    by0 = user_positions(s0, n_users)
    u65 = next(u for u in range(n_users) if by0[u].size == 65)
    s0.items[by0[u65][:5]] = -1
    q_users = np.concatenate([np.arange(n_users), [-1, n_users, n_users + 5], rng.integers(0, n_users, 20)]).astype(np.int32)
    q_users = q_users[rng.permutation(q_users.size)]
    lens = rng.integers(0, 6, q_users.size)
    lens[rng.random(q_users.size) < 0.3] = 0
    extra_rp = np.zeros(q_users.size + 1, np.int64)
    np.cumsum(lens, out=extra_rp[1:])
    extra_ci = np.concatenate([np.sort(rng.choice(n_items, n, replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return Problem(n_users, n_items, streams, q_users, extra_rp, extra_ci)


class DeviceProblem:
    """The problem's streams on the session's device, indexed."""

    def __init__(self, sess, p: Problem, shuffle_index_seed=None):
        self.sess, self.p = sess, p
        self.q_users = self._put(p.q_users)
        self.extra = (self._put(p.extra_rp), self._put(p.extra_ci))
        self.ev = []
        for s in p.streams:
            users = self._put(s.users)
            rp, pos = sess.history_index(users, p.n_users)
            if shuffle_index_seed is not None:    # another order inside every user's segment: what another run's scatter may leave
                sess.synchronize()
                h_rp, h_pos = rp.cpu().numpy(), pos.cpu().numpy().copy()
                rng = np.random.default_rng(shuffle_index_seed)
                for u in range(p.n_users):
                    h_pos[h_rp[u]:h_rp[u + 1]] = rng.permutation(h_pos[h_rp[u]:h_rp[u + 1]])
                pos = self._put(h_pos)
            self.ev.append((s.n_cols, rp, pos, self._put(s.items), self._put(s.times) if s.times is not None else None,
                            self._put(s.col_map) if s.col_map is not None else None))
        self.by_user = [user_positions(s, p.n_users) for s in p.streams]

    def _put(self, a):
        if a.size == 0:
            a = np.zeros(1, a.dtype)                                          # an empty stream still has arrays
        t = self.sess.empty(a.size, torch.from_numpy(a[:0].copy()).dtype)     # the session's allocator: guarded under HIPSIM_GUARD
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return t

    def events(self, caps, blacklist=None):
        bl = blacklist if blacklist is not None else [s.blacklist for s in self.p.streams]
        return [(n_cols, caps[t], bl[t], rp, pos, items, times, cmap) for t, (n_cols, rp, pos, items, times, cmap) in enumerate(self.ev)]


def csr_rows(rp, ci):
    rp = rp.cpu().numpy()
    ci = ci.cpu().numpy()
    return rp, [ci[rp[i]:rp[i + 1]] for i in range(rp.size - 1)]


def check(d: DeviceProblem, caps, use_extra=True, blacklist=None):
    """Runs history_rows and asserts exact equality with the restatement: every term row, every exclusion row, the final row_ptr; every bound >= the final
    length.  Returns (stats, terms, excl) -- the device rows as numpy."""
    p = d.p
    terms, excl, info = d.sess.history_rows(d.q_users, p.n_users, d.events(caps, blacklist), p.n_items, d.extra if use_extra else None, stats=True, keep_bounds=True)
    d.sess.synchronize()
    want_terms, want_excl = rows_ref(p, caps, d.by_user, use_extra, blacklist)
    got = []
    for t in range(len(p.streams) + 1):
        rp_t, ci_t = terms[t] if t < len(p.streams) else excl
        want = want_terms[t] if t < len(p.streams) else want_excl
        rp, rows = csr_rows(rp_t, ci_t)
        want_rp = np.concatenate([[0], np.cumsum([w.size for w in want])])
        assert np.array_equal(rp, want_rp), f"type {t}: final row_ptr differs"
        for q, (g, w) in enumerate(zip(rows, want)):
            assert np.array_equal(g, w), f"type {t}, query {q} (user {p.q_users[q]}): {g[:20]} != {w[:20]}"
        bound = np.diff(info["bound_row_ptr"][t].cpu().numpy())
        assert (bound >= np.diff(rp)).all(), f"type {t}: a bound is below the final length"
        assert info["bounds"][t] == bound.sum()
        got.append(rows)
    stats = info["stats"].cpu().numpy()
    assert stats[6] == 0, stats
    return stats, got[:-1], got[-1]
