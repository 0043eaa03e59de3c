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

I64_MIN, I64_MAX = int(np.iinfo(np.int64).min), int(np.iinfo(np.int64).max)
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
    key_users: Optional[list] = None   # make_key_problem: (user, family, discriminating time bytes, events) per planted user


def user_positions(s: Stream, n_users: int):
    """per user: the stream positions of its events, most recent first"""
    pos = np.arange(s.users.size, dtype=np.int64)
    t = s.times if s.times is not None else np.zeros(s.users.size, np.int64)
    order = np.lexsort((~pos, ~t, s.users))            # by user, then time desc, then position desc; ~x = -x - 1 reverses the order and cannot
    order = order[s.users[order] >= 0]                 # overflow, where -x wraps for INT64_MIN
    u = s.users[order]
    start = np.searchsorted(u, np.arange(n_users + 1))
    return [order[start[i]:start[i + 1]] for i in range(n_users)]


def user_positions_of(s: Stream, who):
    """{u: the stream positions of u's events, most recent first} for the users `who` alone: the stream is filtered first, so a long stream of
    which these users own little costs one pass and no sort of its own"""
    who = np.unique(np.asarray(who, np.int64))
    sel = np.flatnonzero(s.users >= 0)
    sel = sel[np.isin(s.users[sel], who)]
    t = s.times[sel] if s.times is not None else np.zeros(sel.size, np.int64)
    order = sel[np.lexsort((~sel, ~t, s.users[sel]))]
    u = s.users[order]
    return {int(w): order[np.searchsorted(u, w, "left"):np.searchsorted(u, w, "right")] for w in who}


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
    """The problem's streams on the session's device, indexed.  subset: the restatement's positions for these users alone (user_positions_of; every
    other user must be left out of the queries).  host_index: the index of the subset's users is built on the host and the items / times arrays are
    allocated at full length with only those users' entries written -- for a simulator run over a long stream that is almost all nobody's."""

    def __init__(self, sess, p: Problem, shuffle_index_seed=None, subset=None, host_index=False):
        self.sess, self.p = sess, p
        self._put_cache = {}
        self.q_users = self._put(p.q_users)
        self.extra = (self._put(p.extra_rp), self._put(p.extra_ci))
        self.ev = []
        for s in p.streams:
            if host_index:
                by = user_positions_of(s, subset)
                own = [np.sort(by[u]) if u in by else np.zeros(0, np.int64) for u in range(p.n_users)]
                assert sum(o.size for o in own) == np.count_nonzero((s.users >= 0) & (s.users < p.n_users)), "a user outside the subset owns events"
                rng = np.random.default_rng(shuffle_index_seed if shuffle_index_seed is not None else 0)
                h_pos = np.concatenate([rng.permutation(o) for o in own]).astype(np.int32)
                rp = self._put(np.concatenate([[0], np.cumsum([o.size for o in own])]).astype(np.int64))
                pos = self._put(h_pos)
                touched = np.sort(h_pos.astype(np.int64))
                items, times = self._put_at(s.items, touched), self._put_at(s.times, touched) if s.times is not None else None
            else:
                users = self._put(s.users)
                rp, pos = sess.history_index(users, p.n_users)
                if shuffle_index_seed is not None:    # another order inside every user's segment: what another run's scatter may leave
                    sess.synchronize()
                    h_rp, h_pos = rp.cpu().numpy(), pos.cpu().numpy().copy()
                    rng = np.random.default_rng(shuffle_index_seed)
                    for u in range(p.n_users):
                        h_pos[h_rp[u]:h_rp[u + 1]] = rng.permutation(h_pos[h_rp[u]:h_rp[u + 1]])
                    pos = self._put(h_pos)
                items, times = self._put(s.items), self._put(s.times) if s.times is not None else None
            self.ev.append((s.n_cols, rp, pos, items, times, self._put(s.col_map) if s.col_map is not None else None))
        self.by_user = [user_positions(s, p.n_users) if subset is None else user_positions_of(s, subset) for s in p.streams]

    @classmethod
    def over(cls, sess, p: Problem, ev):
        """The problem over streams and indexes that already live on the device -- ev: per stream (n_cols, idx_row_ptr, idx_pos, items, times | None,
        col_map | None), e.g. the live tensors of a DeviceHistory; only the queries and the extra rows are copied"""
        d = cls.__new__(cls)
        d.sess, d.p, d._put_cache = sess, p, {}
        d.q_users = d._put(p.q_users)
        d.extra = (d._put(p.extra_rp), d._put(p.extra_ci))
        d.ev = list(ev)
        assert len(d.ev) == len(p.streams)
        d.by_user = [user_positions(s, p.n_users) for s in p.streams]
        return d

    def _put(self, a):
        if id(a) in self._put_cache:              # streams may share an array (two event types over one stream): one copy on the device
            return self._put_cache[id(a)][1]
        src = a
        if a.size == 0:
            a = np.zeros(1, a.dtype)                                          # an empty stream still has arrays
        t = self.sess.empty(a.size, torch.from_numpy(a[:0].copy()).dtype)     # the session's allocator: guarded under HIPSIM_GUARD
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        self._put_cache[id(src)] = (src, t)
        return t

    def _put_at(self, a, idx):
        """full length, only a[idx] written (host sessions: the rest of the pages is never touched)"""
        if (id(a), "at") in self._put_cache:
            return self._put_cache[(id(a), "at")][1]
        t = self.sess.empty(a.size, torch.from_numpy(a[:0].copy()).dtype)
        t[torch.from_numpy(idx)] = torch.from_numpy(a[idx])
        self._put_cache[(id(a), "at")] = (a, t)
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


# ---- the key domain: which bytes of the 96-bit key (time ^ sign bit, position) tell a user's events apart ---------------------------------------
KEY_V = (0, 1, 127, 128, 255)                     # values of a discriminating byte: few, so ties are the rule
KEY_POS = 0x00017F80FF000180                      # every byte of both bases is one of KEY_V: base byte ^ v reaches 0, the lowest bucket of a digit pass
KEY_NEG = 0xFF8001007FFF8001 - (1 << 64)
KEY_SPECIALS = (I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX)
KEY_CAPS = (1, 20, 39, 63, 64, 150, 299, 2048, 4095, 4096, 5999)   # 1, n_u - 1 and about n_u / 2 of the planted event counts below


def family_times(rng, family, n):
    """int64 times of n events of one user.  family: ("byte", b, base) -- base ^ (v << 8b), v from KEY_V; ("two", base) -- bytes 6 and 1 vary, the
    bytes between them do not; ("full",) -- uniform over int64 from raw bits with KEY_SPECIALS planted twice each (n >= 12); ("equal", base)"""
    v = np.array(KEY_V, np.uint64)
    if family[0] == "byte":
        t = np.uint64(family[2] & (2**64 - 1)) ^ (v[rng.integers(0, v.size, n)] << np.uint64(8 * family[1]))
    elif family[0] == "two":
        t = np.uint64(family[1] & (2**64 - 1)) ^ (v[rng.integers(0, v.size, n)] << np.uint64(48)) ^ (v[rng.integers(0, v.size, n)] << np.uint64(8))
    elif family[0] == "full":
        t = rng.integers(0, 2**64, n, dtype=np.uint64)
        where = rng.permutation(n)[: 2 * len(KEY_SPECIALS)]
        t[where] = np.array(KEY_SPECIALS * 2, dtype=np.int64).view(np.uint64)
    else:
        t = np.full(n, family[1] & (2**64 - 1), np.uint64)
    return t.view(np.int64)


def key_bytes(family):
    """the time bytes (0 = least significant) in which the family's times differ"""
    return {"byte": lambda: (family[1],), "two": lambda: (6, 1), "full": lambda: tuple(range(8)), "equal": lambda: ()}[family[0]]()


def _queries(rng, n_users, n_items):
    q_users = np.concatenate([np.arange(n_users), [-1, n_users, n_users + 5], rng.integers(0, n_users, 10)]).astype(np.int32)
    q_users = q_users[rng.permutation(q_users.size)]
    lens = rng.integers(0, 6, q_users.size)
    lens[rng.random(q_users.size) < 0.3] = 0
    extra_rp = np.zeros(q_users.size + 1, np.int64)
    np.cumsum(lens, out=extra_rp[1:])
    extra_ci = np.concatenate([np.sort(rng.choice(n_items, n, replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return q_users, extra_rp, extra_ci


def make_key_problem(seed=11):
    """One event type with times and one without.  Every planted user of type 0 takes its times from one family (family_times): per byte b = 0..7 a
    user of the wave class, one of the block class and one of the global class, over a positive and a negative base (b = 7 straddles the sign bit);
    two discriminating bytes around uniform ones; the full int64 domain; all times equal.  40 / 64 | 65 / 300 / 4096 | 4097 / 6000 events.  Items from
    2^20 columns, so a term row is (almost) its window: a wrong window shows.  Type 1: stream order alone, 65 and 300 events planted."""
    rng = np.random.default_rng(seed)
    n_cols = 1 << 20
    plan = []
    for b in range(8):
        a, o = (KEY_POS, KEY_NEG) if b % 2 == 0 else (KEY_NEG, KEY_POS)
        plan += [(("byte", b, a), 40 if b % 2 else 64), (("byte", b, o), 300 if b % 2 else 65), (("byte", b, a), 4097)]
    plan += [(("byte", 7, KEY_POS), 300), (("byte", 7, KEY_NEG), 64), (("byte", 7, KEY_NEG), 4097), (("byte", 4, KEY_POS), 4096)]
    plan += [(("two", KEY_NEG), 64), (("two", KEY_POS), 300), (("two", KEY_NEG), 4097)]
    plan += [(("full",), 40), (("full",), 65), (("full",), 4096), (("full",), 6000)]
    plan += [(("equal", KEY_NEG), 40), (("equal", KEY_POS), 300), (("equal", KEY_NEG), 4097)]
    n_users = len(plan) + 4                                       # the last users own nothing
    who = rng.permutation(n_users)[: len(plan)]
    users = np.concatenate([np.repeat(who, [n for _, n in plan]).astype(np.int32), np.full(5, -1, np.int32)])
    times = np.concatenate([family_times(rng, f, n) for f, n in plan] + [np.zeros(5, np.int64)])
    order = rng.permutation(users.size)
    users, times = users[order], times[order]
    items = rng.integers(0, n_cols, users.size).astype(np.int32)
    items[rng.random(users.size) < 0.03] = -1
    streams = [Stream(n_cols, users, items, times, None, True)]
    counts = rng.integers(0, 31, n_users)
    counts[who[:2]] = (65, 300)
    users1 = np.repeat(np.arange(n_users, dtype=np.int32), counts)
    users1 = users1[rng.permutation(users1.size)]
    col_map = rng.integers(0, n_cols, 50).astype(np.int32)
    col_map[rng.random(50) < 0.3] = -1
    streams.append(Stream(50, users1, rng.integers(-1, 50, users1.size).astype(np.int32), None, col_map, True))
    q_users, extra_rp, extra_ci = _queries(rng, n_users, n_cols)
    key_users = [(int(u), f, key_bytes(f), n) for u, (f, n) in zip(who, plan)]
    return Problem(n_users, n_cols, streams, q_users, extra_rp, extra_ci, key_users)


def _class_of(n):
    return 0 if n <= 64 else 1 if n <= 4096 else 2


def assert_key_edge_cases(p: Problem, caps=KEY_CAPS):
    """From the restatement alone: what make_key_problem promises, for the caps a test runs it with."""
    s = p.streams[0]
    by = user_positions(s, p.n_users)
    assert 60000 < s.users.size < 70000 and p.streams[1].times is None
    key = s.times.view(np.uint64) ^ np.uint64(1 << 63)            # the order-preserving unsigned form
    differs = {(c, b): False for c in range(3) for b in range(8)}                     # (class, byte b): a select over keys that differ in byte b alone
    bucket = {(c, w): False for c in range(3) for w in ("top", "middle", "zero")}      # where the cap-th key falls in the first digit pass
    cut_in_run = {f[0]: False for _, f, _, _ in p.key_users}
    signs = set()
    for u, family, bts, n in p.key_users:
        ev = by[u]
        assert ev.size == n
        k = key[ev]
        diff = int(np.bitwise_or.reduce(k ^ k[0]))
        assert {b for b in range(8) if (diff >> (8 * b)) & 255} == set(bts), (family, hex(diff))
        if family[0] == "full":
            for x in KEY_SPECIALS:
                assert np.count_nonzero(s.times[ev] == x) >= 2, x
        assert [int(x) for x in ev] == sorted((int(x) for x in ev), key=lambda q: (int(s.times[q]), q), reverse=True)
        for cap in caps:
            if cap >= n:
                continue
            w = s.times[ev[:cap]]
            signs.add("neg" if (w < 0).all() else "pos" if (w >= 0).all() else "mixed")
            cut_in_run[family[0]] |= bool(s.times[ev[cap - 1]] == s.times[ev[cap]])
            if bts:
                top = max(bts)
                digit = (k >> np.uint64(8 * top)) & np.uint64(255)
                d = int(digit[cap - 1])
                where = "top" if d == int(digit.max()) else "zero" if d == 0 else "middle" if d > int(digit.min()) else None
                if where:
                    bucket[(_class_of(n), where)] = True
            if family[0] == "byte":
                differs[(_class_of(n), family[1])] = True
    assert all(differs.values()), [k for k, v in differs.items() if not v]
    assert all(bucket.values()), [k for k, v in bucket.items() if not v]
    assert all(cut_in_run.values()), cut_in_run
    assert signs == {"neg", "pos", "mixed"}, signs
    for c, sizes in enumerate(((40, 64), (65, 300, 4096), (4097, 6000))):
        assert 1 in caps and all(n - 1 in caps for n in sizes) and any(_class_of(n) == c for _, _, _, n in p.key_users)
    n1 = np.array([r.size for r in user_positions(p.streams[1], p.n_users)])
    assert (n1 == 65).any() and (n1 == 300).any() and (n1 == 0).any()


def make_byte0_job(seed=2):
    """One user, 300 events whose times differ in the lowest byte alone, one query: one job of the block class"""
    rng = np.random.default_rng(seed)
    times = (1_600_000_000_000 + rng.integers(0, 50, 300)).astype(np.int64)
    s = Stream(1 << 20, np.zeros(300, np.int32), rng.integers(0, 1 << 20, 300).astype(np.int32), times, None, True)
    return Problem(1, 1 << 20, [s], np.zeros(1, np.int32), np.zeros(2, np.int64), np.zeros(0, np.int32))


# ---- stream positions at and beyond 2^24: the most significant position digit decides ------------------------------------------------------------
FAR = 1 << 24
FAR_EVENTS = FAR + (1 << 16)
FAR_USERS = ((40, 13), (65, 30), (300, 100), (4097, 2000), (5000, 3100))     # (events, of them at or above 2^24) per user


def make_far_problem(seed=23):
    """One stream of 2^24 + 2^16 events, almost all nobody's; FAR_USERS own a few on both sides of position 2^24 (2^24 - 1, 2^24 and 2^24 + 1 among
    them).  Two event types over the SAME arrays: without times, and with all times equal -- the positions alone decide."""
    rng = np.random.default_rng(seed)
    users = np.full(FAR_EVENTS, -1, np.int32)
    items = np.zeros(FAR_EVENTS, np.int32)
    edge = [FAR - 1, FAR, FAR + 1]                          # user 2's, among its 300
    near = [FAR - 2, FAR + 2, FAR - 3, FAR + 3]             # the neighbours of the edge go to the global-class users 3, 4, 4, 3 on top of their events
    free_hi = np.setdiff1d(np.arange(FAR, FAR_EVENTS), edge + near)
    free_lo = np.setdiff1d(np.concatenate([np.arange(0, 1 << 15), np.arange(FAR - (1 << 15), FAR)]), edge + near)
    free_hi, free_lo = free_hi[rng.permutation(free_hi.size)], free_lo[rng.permutation(free_lo.size)]
    for u, (n, hi) in enumerate(FAR_USERS):
        take_hi, take_lo = hi - (2 if u == 2 else 0), n - hi - (1 if u == 2 else 0)
        pos = np.concatenate([np.array(edge if u == 2 else [], np.int64), free_hi[:take_hi], free_lo[:take_lo]])
        free_hi, free_lo = free_hi[take_hi:], free_lo[take_lo:]
        users[pos] = u
    users[near] = (3, 4, 4, 3)
    mine = np.flatnonzero(users >= 0)
    items[mine] = rng.integers(0, 1 << 20, mine.size)
    times = np.full(FAR_EVENTS, KEY_NEG, np.int64)
    n_users = len(FAR_USERS) + 1
    streams = [Stream(1 << 20, users, items, None, None, True), Stream(1 << 20, users, items, times, None, False)]
    q_users = np.array([0, 1, 2, 3, 4, 5, -1, 3, n_users], np.int32)
    return Problem(n_users, 1 << 20, streams, q_users, np.zeros(q_users.size + 1, np.int64), np.zeros(0, np.int32))


def far_caps(p: Problem):
    """per user the number h of its events at or above 2^24 -> caps h - 1, h, h + 1"""
    u = p.streams[0].users
    hs = [int(np.count_nonzero(u[FAR:] == w)) for w in range(len(FAR_USERS))]
    lo = [int(np.count_nonzero(u[:FAR] == w)) for w in range(len(FAR_USERS))]
    assert all(h >= 2 and l >= 2 for h, l in zip(hs, lo)), (hs, lo)          # events on both sides, every cap cuts inside the user's events
    assert u[FAR - 1] == u[FAR] == u[FAR + 1] == 2
    return sorted({h + d for h in hs for d in (-1, 0, 1)})


# ---- the capacity contract of urcco_dev_history_rows ---------------------------------------------------------------------------------------------
SENTINEL = -77


def rows_with_capacity(d: DeviceProblem, caps, capacity, pad=0):
    """urcco_dev_history_bounds, then urcco_dev_history_rows with the capacities capacity(t, bound_row_ptr) (t == n_types: the exclusion rows), through
    ctypes.  The col_idx arrays hold max(capacity, 1) + pad entries from the session's allocator, filled with SENTINEL.  Returns (bound row_ptr arrays,
    capacities, final row_ptr arrays, col_idx arrays, stats), numpy, the exclusion rows last."""
    from universal_recommender_amd import _lib
    s, p = d.sess, d.p
    nq, nt = d.q_users.numel(), len(p.streams)
    arr = (_lib.HistEvent * nt)()
    rps = [s.empty(nq + 1, torch.int64) for _ in range(nt + 1)]
    for t, (n_cols, cap, bl, irp, ipos, items, times, cmap) in enumerate(d.events(caps)):
        arr[t].n_cols, arr[t].max_items, arr[t].blacklist = n_cols, cap, int(bl)
        arr[t].idx_row_ptr, arr[t].idx_pos, arr[t].items = irp.data_ptr(), ipos.data_ptr(), items.data_ptr()
        arr[t].times_ms, arr[t].col_map = times.data_ptr() if times is not None else None, cmap.data_ptr() if cmap is not None else None
        arr[t].term_row_ptr = rps[t].data_ptr()
    args = (s.handle, nq, d.q_users.data_ptr(), p.n_users, arr, nt, d.extra[0].data_ptr(), d.extra[1].data_ptr())
    assert s.lib.urcco_dev_history_bounds(*args, rps[nt].data_ptr()) == _lib.OK
    s.synchronize()
    bound = [rp.cpu().numpy().copy() for rp in rps]
    capacities = [int(capacity(t, bound[t])) for t in range(nt + 1)]
    cis = []
    for t, c in enumerate(capacities):
        ci = s.empty(max(c, 1) + pad, torch.int32)
        ci.fill_(SENTINEL)
        cis.append(ci)
        if t < nt:
            arr[t].term_col_idx, arr[t].term_capacity = ci.data_ptr(), c
    st = s.empty(_lib.HIST_STATS_LEN, torch.int64)
    assert s.lib.urcco_dev_history_rows(*args, p.n_items, rps[nt].data_ptr(), cis[nt].data_ptr(), capacities[nt], st.data_ptr()) == _lib.OK
    s.synchronize()
    return bound, capacities, [rp.cpu().numpy() for rp in rps], [ci.cpu().numpy() for ci in cis], st.cpu().numpy()


def check_capacity(d: DeviceProblem, caps, capacity, pad=0):
    """The contract of include/urcco.h for capacities below the bounds: a row is served iff the END of its bound (row_ptr[q + 1] after _bounds) is within
    the capacity; served rows equal the restatement, the others are empty and counted in stats[6]; stats[0..5] count served rows only; nothing is
    written at or past the capacity.  Returns the number of rows dropped per type."""
    p = d.p
    nt = len(p.streams)
    bound, capacities, rps, cis, stats = rows_with_capacity(d, caps, capacity, pad)
    want_terms, want_excl = rows_ref(p, caps, d.by_user)
    known = (p.q_users >= 0) & (p.q_users < p.n_users)
    want_stats = np.zeros(8, np.int64)
    dropped = []
    for t in range(nt + 1):
        want = want_terms[t] if t < nt else want_excl
        served = bound[t][1:] <= capacities[t]
        assert (np.diff(served.astype(int)) <= 0).all()                       # the bound ends ascend: the served rows are a prefix
        lens = np.array([w.size if ok else 0 for w, ok in zip(want, served)], np.int64)
        assert np.array_equal(rps[t], np.concatenate([[0], np.cumsum(lens)])), f"type {t}: the final row_ptr is not the scan of the served rows' lengths"
        for q, (w, ok) in enumerate(zip(want, served)):
            g = cis[t][rps[t][q]:rps[t][q + 1]]
            assert np.array_equal(g, w if ok else w[:0]), f"type {t}, query {q}, served {ok}: {g[:20]} != {w[:20]}"
        assert (cis[t][capacities[t]:] == SENTINEL).all(), f"type {t}: written at or past the capacity {capacities[t]}"
        if t < nt:
            n_u = np.array([d.by_user[t][u].size if k else 0 for u, k in zip(p.q_users, known)])
            assert np.array_equal(np.diff(bound[t]), np.minimum(n_u, caps[t]))
            for c, sel in enumerate((n_u <= 64, (n_u > 64) & (n_u <= 4096), n_u > 4096)):
                want_stats[c] += np.count_nonzero(served & sel)
            want_stats[3] += np.count_nonzero(served & (n_u > caps[t]))
        else:
            raw = np.diff(bound[t])
            want_stats[4] += np.count_nonzero(served & (raw <= 64))
            want_stats[5] += np.count_nonzero(served & (raw > 64))
        want_stats[6] += np.count_nonzero(~served)
        dropped.append(int(np.count_nonzero(~served)))
    assert np.array_equal(stats, want_stats), (stats, want_stats)
    return dropped


def capacity_cases(d: DeviceProblem, caps, pad=0):
    """The three cases of the capacity tests on make_problem(): a cut at a middle query with the heavy user and block-class jobs behind it; capacity 0
    for one type only; every capacity one below its bound total."""
    p = d.p
    nq = p.q_users.size
    n0 = np.array([d.by_user[0][u].size if 0 <= u < p.n_users else 0 for u in p.q_users])
    heavy_q = int(np.flatnonzero(n0 == n0.max())[0])
    qm = min(nq // 2, heavy_q)
    assert qm > nq // 8 and np.count_nonzero((n0[qm:] > 64) & (n0[qm:] <= 4096)) >= 3, (qm, heavy_q)
    dropped = check_capacity(d, caps, lambda t, rp: rp[qm], pad)
    assert all(x >= nq - qm for x in dropped), dropped
    dropped = check_capacity(d, caps, lambda t, rp: 0 if t == 1 else rp[-1], pad)
    assert dropped[0] == 0 and dropped[1] > 0 and dropped[2] == 0 and dropped[3] == 0, dropped
    dropped = check_capacity(d, caps, lambda t, rp: rp[-1] - 1, pad)
    assert all(1 <= x < nq // 2 for x in dropped), dropped


# ---- DeviceHistory.from_streams against the dict form --------------------------------------------------------------------------------------------
def predict_stack(sess, n_rows, n_items, n_view, caps=(6, 70)):
    """A device-built model over integer ids, two event types, and its algorithm object"""
    from helpers import rand_csr, run_device
    from oracle import c_oracle as O
    from universal_recommender_amd.recommend import DeviceModel
    from universal_recommender_amd.ur_algorithm import URAlgorithm, URAlgorithmParams
    rng = np.random.default_rng(31)
    mats = [rand_csr(rng, n_rows, n_items, 8), rand_csr(rng, n_rows, n_view, 10)]
    out = run_device(sess, mats, [O.DatasetParams(100, 20, None)] * 2, 7)
    model = DeviceModel.from_indicators(sess, [("purchase", out[0]), ("view", out[1])], properties={})
    engine = {"algorithms": [{"name": "ur", "params": {"appName": "t", "indexName": "t", "typeName": "items", "num": 10,
                                                       "indicators": [{"name": "purchase", "maxItemsPerUser": caps[0]}, {"name": "view", "maxItemsPerUser": caps[1]}]}}]}
    return URAlgorithm(URAlgorithmParams.from_engine_json(engine), device=0, library=sess.lib), model


def make_stream_history(seed, n_users, n_items, n_view, max_events=150):
    """Event streams in shuffled order and the dict that says the same.  "purchase": int64 times per user from the families of make_key_problem
    (negative times and ties among them), ids up to 5 % beyond the items; "view": no times.  Users 0..n_users-3 own 0..max_events events per type, the
    last two none.  Returns ({event: (users int32, items int32 (-1: outside the dictionary), times | None)}, {user: {event: [ids, oldest first]}})."""
    rng = np.random.default_rng(seed)
    families = [("byte", b, base) for b in range(8) for base in (KEY_POS, KEY_NEG)] + [("two", KEY_NEG), ("full",), ("equal", KEY_POS)]
    streams, history = {}, {u: {} for u in range(n_users - 2)}
    for ev, hi, n_cols in (("purchase", n_items + n_items // 20, n_items), ("view", n_view, n_view)):
        counts = rng.integers(0, max_events, n_users)
        counts[-2:] = 0
        counts[:3] = (max_events, 12, 0)
        users = np.repeat(np.arange(n_users, dtype=np.int32), counts)
        times = None
        if ev == "purchase":
            times = np.concatenate([family_times(rng, families[u % len(families)] if c >= 12 else ("equal", 5), c) for u, c in enumerate(counts)] + [np.zeros(0, np.int64)])
        order = rng.permutation(users.size)
        users, times = users[order], times[order] if times is not None else None
        ids = rng.integers(0, hi, users.size)
        for u in history:
            pos = [int(q) for q in np.flatnonzero(users == u)]
            pos.sort(key=(lambda q: (int(times[q]), q)) if times is not None else None)          # oldest first; equal times: stream order
            history[u][ev] = [int(ids[q]) for q in pos]
        streams[ev] = (users, np.where(ids < n_cols, ids, -1).astype(np.int32), times)
    return streams, history


def check_from_streams(sess, algo, model, n_users, streams, history):
    """batch_predict with DeviceHistory.from_streams == batch_predict with the dict, for both ways of resolving users and blacklistEvents in
    (None, [], [...]); the ValueErrors of from_streams"""
    import pytest
    from universal_recommender_amd.history import DeviceHistory
    dev = {ev: tuple(torch.from_numpy(a).to(sess.device) if a is not None else None for a in st) for ev, st in streams.items()}
    assert dev["purchase"][2].dtype == torch.int64 and bool((dev["purchase"][2] < 0).any()) and dev["view"][2] is None
    names = {f"user-{u}": u for u in range(n_users)}
    by_id = DeviceHistory.from_streams(sess, model, dev)
    assert by_id.n_users == n_users - 2 and by_id.user_index(n_users - 1) == -1 and by_id.user_index(1) == 1      # the default: the largest id + 1
    by_name = DeviceHistory.from_streams(sess, model, dev, user_ids=names)
    assert by_name.n_users == n_users and by_name.user_index("user-3") == 3 and by_name.user_index(3) == -1
    explicit = DeviceHistory.from_streams(sess, model, dev, n_users=n_users + 7)
    assert explicit.n_users == n_users + 7
    for dh, name in ((by_id, lambda u: u), (by_name, lambda u: f"user-{u}"), (explicit, lambda u: u)):
        hist = {name(u): h for u, h in history.items()}
        us = list(range(n_users))
        qs = [{"user": name(u)} for u in us] + [{"user": name(u), "item": int(u * 2)} for u in us[1::7]]
        qs += [{"user": name(u), "userBias": -1.0, "num": 5} for u in us[2::5]] + [{"user": name(u), "blacklistItems": [1, 2, 3], "from": 2, "num": 4} for u in us[::4]]
        qs += [{"user": name(n_users + 100)}, {}, {"item": 5}]
        for blacklist in (None, [], ["purchase", "view"]):
            algo.ap.blacklistEvents = blacklist
            want = algo.batch_predict(model, qs, hist)
            got = algo.batch_predict(model, qs, dh)
            for q, w, g in zip(qs, want, got):
                assert g == w, (blacklist, q, g, w)
        assert any(s["score"] > 0 for r in want for s in r["itemScores"])
    algo.ap.blacklistEvents = None
    u, i, t = dev["purchase"]
    for bad in ((u.to(torch.int64), i, t), (u, i.to(torch.int64), t), (u[:-1], i, t), (u, i, t.to(torch.int32)), (u, i, t[:-1]), (u, i[:-1], None)):
        with pytest.raises(ValueError):
            DeviceHistory.from_streams(sess, model, {"purchase": bad})
