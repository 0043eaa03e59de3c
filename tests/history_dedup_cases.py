"""urcco_dev_history_dedup (decision D29 of DESIGN.md, include/urcco.h): the problems and checks that tests/test_sim_history_dedup.py and
tests/test_gpu_history_dedup.py share.  The contract in numpy: history_trim_cases.trim_ref with one more rule (dup_ref).  Every output buffer has exactly the
restatement's size, so the rerun under HIPSIM_GUARD faults on an access past it.  HD = HD_LDS (csrc/cco_kernels.h, restated in _lib): the LDS class's bound."""
import os

import numpy as np
import torch

import history_cap_cases as C
import history_lifecycle_cases as L
import history_ref as H
import history_trim_cases as T
from history_append_cases import put, row_ptr_ref
from universal_recommender_amd import _lib

I64_MIN, T0, SENTINEL, HD = H.I64_MIN, T.T0, T.SENTINEL, _lib.HD_LDS
KEEPS = {"first": _lib.DEDUP_FIRST, "last": _lib.DEDUP_LAST}
LENGTHS = (0, 1, 2, 63, 64, 65, HD - 1, HD, HD + 1, 2 * HD + 1)
NONE = np.zeros(0, np.int32)


def dup_ref(t: T.TrimProblem, n_cols, keep):
    """bool [n_events]: the positions the duplicate rule drops (row starts monotone; entries outside the stream allowed)"""
    n, out = t.n_events, np.zeros(t.n_events, bool)
    if t.n_users == 0 or n == 0:
        return out
    rp = np.clip(t.row_ptr, 0, min(max(int(t.row_ptr[-1]), 0), n))
    user, p = np.repeat(np.arange(t.n_users), np.diff(rp)), t.pos[rp[0]:rp[-1]].astype(np.int64)
    ok = (p >= 0) & (p < n)
    q = np.where(ok, p, 0)
    ok &= (t.items[q] >= 0) & (t.items[q] < n_cols) & (True if t.times is None else t.times[q] >= t.min_time)
    user, p = user[ok], p[ok]
    tk = t.times[p].view(np.uint64) ^ C.SIGN if t.times is not None else np.zeros(p.size, np.uint64)
    order = np.lexsort((p, tk, t.items[p], user))
    user, item, p = user[order], t.items[p][order], p[order]
    new = np.r_[True, (user[1:] != user[:-1]) | (item[1:] != item[:-1])][: p.size]      # the first of its (user, item) group
    out[p[~(new if keep == "first" else np.r_[new[1:], True])]] = True
    return out


def run_dedup(sess, t: T.TrimProblem, n_cols, keep, sizes, null=()):
    """One call, the outputs at exactly sizes = (K, KE) entries (one where that is 0); null: arguments passed as NULL.  Returns (status, the five outputs)."""
    k, ke, timed = int(sizes[0]), int(sizes[1]), t.times is not None
    a = dict(items=put(sess, t.items), times=(put(sess, t.times) if t.n_events else sess.empty(1, torch.int64)) if timed else None, rp=put(sess, t.row_ptr),
             pos=put(sess, t.pos) if t.pos.size or not t.n_events else sess.empty(1, torch.int32), drop=put(sess, t.drop), o_items=sess.empty(max(k, 1), torch.int32),
             o_times=sess.empty(max(k, 1), torch.int64) if timed else None, o_rp=sess.empty(t.n_users + 1, torch.int64), o_pos=sess.empty(max(ke, 1), torch.int32),
             counts=sess.empty(2, torch.int64))
    for name in ("o_items", "o_times", "o_rp", "o_pos", "counts"):
        if a[name] is not None:
            a[name].fill_(SENTINEL)
    p = {name: x.data_ptr() if x is not None and x.numel() and name not in null and (name != "rp" or t.n_users) else None for name, x in a.items()}      # no entries: NULL
    status = sess.lib.urcco_dev_history_dedup(None if "s" in null else sess.handle, t.n_events, p["items"], p["times"], t.n_users, p["rp"], p["pos"], t.min_time, t.drop.size,
                                              p["drop"], n_cols, KEEPS.get(keep, keep), p["o_items"], p["o_times"], p["o_rp"], p["o_pos"], p["counts"])
    sess.synchronize()
    return (status,) + tuple(a[name].cpu().numpy() if a[name] is not None else None for name in ("o_items", "o_times", "o_rp", "o_pos", "counts"))


def check_dedup(sess, t: T.TrimProblem, n_cols, keep):
    """The call against trim_ref over the problem whose time rule is "time rule and not dup": the five outputs, bit for bit.  Returns the kept positions."""
    ok = (np.ones(t.n_events, bool) if t.times is None else t.times >= t.min_time) & ~dup_ref(t, n_cols, keep)
    kept, _, w_items, _, w_rp, w_pos, w_counts = T.trim_ref(T.TrimProblem(t.name, t.n_users, t.items, ok.astype(np.int64), t.row_ptr, t.pos, 1, t.drop))
    w_times = t.times[kept] if t.times is not None else None
    status, items, times, rp, pos, counts = run_dedup(sess, t, n_cols, keep, w_counts)
    name, k, ke = f"{t.name} {keep}", int(w_counts[0]), int(w_counts[1])
    assert status == _lib.OK and np.array_equal(counts, w_counts), (name, status, counts, w_counts)
    assert np.array_equal(items[:k], w_items) and (times is None) == (w_times is None) and (times is None or np.array_equal(times[:k], w_times)), name
    assert np.array_equal(rp, w_rp) and np.array_equal(pos[:ke], w_pos), name
    return kept


def make_problem(counts, items, times, seed, **kw):
    """history_cap_cases.make_problem (a shuffled stream, a random order inside every segment, 5 positions of nobody) with every user's m items drawn by
    pattern: one item; all distinct; every item twice; multiples of 4096 (one probe chain under any low-bits mask); m - 1 distinct items and one repeat
    (m == HD: the table at its load bound).  Returns (problem, users, n_cols)."""
    t, users = C.make_problem(list(counts), times, seed, **kw)
    rng = np.random.default_rng(seed)
    for u in range(t.n_users):
        seg = t.pos[t.row_ptr[u]:t.row_ptr[u + 1]]
        i = np.arange(seg.size)
        v = {"one": np.full(seg.size, 7), "distinct": i, "twice": i // 2, "chain": 4096 * (i % 37), "load": np.where(i == seg.size - 1, 0, i)}[items]
        t.items[seg] = v[rng.permutation(seg.size)]
    t.name = f"{items} / {times} {seed}"
    return t, users, int(t.items.max()) + 1


def segment_case(sess, keep, items, times):
    t, users, n_cols = make_problem((0,) + LENGTHS + (0, 3), items, times, 200 + len(items) + len(times))
    check_dedup(sess, t, n_cols, keep)


def column_table_case(sess, keep):
    """one user owns 100 000 of 100 100 events over 300 columns; then, under a zero table budget (read per call), ONE block serves three users beyond HD"""
    rng = np.random.default_rng(5)
    big, n = C.BIG_OWNER
    old = os.environ.get("URCCO_HD_TABLE_BUDGET")
    try:
        for counts, budget in (([3, big, 0, n - big - 8], None), ([HD + 1, 40, 3 * HD, 2 * HD + 77, 70], "0")):
            os.environ.update(URCCO_HD_TABLE_BUDGET=budget) if budget else os.environ.pop("URCCO_HD_TABLE_BUDGET", None)
            for times in ("ties", "none"):
                t, users = C.make_problem(counts, times, 11 + len(counts))
                t.items = rng.integers(0, 300, t.n_events).astype(np.int32)
                check_dedup(sess, t, 300, keep)
    finally:
        os.environ.update(URCCO_HD_TABLE_BUDGET=old) if old is not None else os.environ.pop("URCCO_HD_TABLE_BUDGET", None)


def index_order_case(sess, keep):
    """the same stream under three indexes that differ in the order inside the segments (random, ascending, descending): the same kept events"""
    t, users, n_cols = make_problem([70, 5, 64, 65, 700, HD + 9, 1], "twice", "ties", 41)
    asc = np.flatnonzero(users >= 0)
    asc = asc[np.argsort(users[asc], kind="stable")].astype(np.int32)
    desc = np.concatenate([asc[t.row_ptr[u]:t.row_ptr[u + 1]][::-1] for u in range(t.n_users)])
    kept = [check_dedup(sess, T.TrimProblem(t.name, t.n_users, t.items, t.times, t.row_ptr, p, t.min_time, t.drop), n_cols, keep) for p in (t.pos, asc, desc)]
    assert np.array_equal(kept[0], kept[1]) and np.array_equal(kept[0], kept[2]) and not kept[0].all()


def no_column_case(sess, keep):
    """items of -1 and n_cols among the duplicates: they are kept and shadow nothing"""
    t, users, n_cols = make_problem([0, 2, 40, 64, 300, HD, HD + 50], "twice", "ties", 47)
    out = np.random.default_rng(3).random(t.n_events) < 0.3
    t.items[out] = np.where(np.arange(t.n_events) % 2, -1, n_cols)[out]
    kept = check_dedup(sess, t, n_cols, keep)
    assert kept[out].all() and not kept[~out].all()


def time_cut_case(sess, keep):
    """a cut that removes would-be FIRST winners; one call with the cut, listed users and the duplicates == trim then dedup; dedup twice == once"""
    t, users, n_cols = make_problem([0, 70, 64, 65, 700, HD + 200, 30, 1, 2 * HD], "twice", "ties", 53, min_time=T0, drop=(4, 6, 99))
    kept = check_dedup(sess, t, n_cols, keep)
    uncut = ~dup_ref(T.TrimProblem("", t.n_users, t.items, t.times, t.row_ptr, t.pos, I64_MIN, NONE), n_cols, "first") & (users >= 0)      # FIRST's winners without the cut
    assert (uncut & (t.times < T0)).any() and (keep == "last" or (kept & ~uncut & (users >= 0)).any())
    d = [put(sess, x) for x in (t.items, t.times, t.row_ptr, t.pos, t.drop)]
    one = sess.history_dedup(t.n_events, *d[:4], n_cols, keep, t.min_time, d[4])
    a = sess.history_trim(t.n_events, *d[:4], t.min_time, d[4])
    sess.synchronize()
    k, ke = one[4].tolist()
    assert k == np.count_nonzero(kept) and 0 < ke < k < t.n_events
    for x in (sess.history_dedup(int(a[4][0]), *a[:4], n_cols, keep), sess.history_dedup(k, *one[:4], n_cols, keep)):
        sess.synchronize()
        assert x[4].tolist() == [k, ke] and all(torch.equal(g[:c], w[:c]) for g, w, c in zip(x[:4], one[:4], (k, k, t.n_users + 1, ke)))


def degenerate_case(sess, keep):
    """no users, no events, nothing at all, most positions nobody's"""
    rng = np.random.default_rng(61)
    n = 200
    items, times = rng.integers(0, 5, n).astype(np.int32), (T0 + rng.integers(-5, 5, n)).astype(np.int64)
    assert np.array_equal(check_dedup(sess, T.TrimProblem("no users", 0, items, times, np.zeros(1, np.int64), NONE, T0, NONE), 5, keep), times >= T0)
    check_dedup(sess, T.TrimProblem("no events", 4, NONE, np.zeros(0, np.int64), np.zeros(5, np.int64), NONE, T0, np.array([1], np.int32)), 5, keep)
    check_dedup(sess, T.TrimProblem("nothing at all", 0, NONE, None, np.zeros(1, np.int64), NONE, T0, NONE), 3, keep)
    users = np.full(n, -1, np.int32)
    users[rng.permutation(n)[:40]] = 2
    kept = check_dedup(sess, T.TrimProblem("nobody's", 5, items, times, *T.host_index(users, 5, rng), I64_MIN, NONE), 5, keep)
    assert kept[users < 0].all() and np.count_nonzero(kept) == n - 40 + 5


def hostile_case(sess, keep):
    """Whatever idx_row_ptr and idx_pos hold: URCCO_OK, the run ends, no access leaves the arrays (HIPSIM_GUARD), 0 <= KE <= K <= n_events"""
    rng = np.random.default_rng(67)
    counts = [2 * HD + 100, 40, 700, 65, 64, 63, 1, 0, HD, 100, 20, 7]
    n, n_users = sum(counts), len(counts)
    users = np.repeat(np.arange(n_users, dtype=np.int32), counts)[rng.permutation(n)]
    rp, pos = T.host_index(users, n_users, rng)
    items, times = rng.integers(-1, 51, n).astype(np.int32), (T0 + rng.integers(-20, 20, n)).astype(np.int64)
    bad_pos = pos.copy()
    bad_pos[rng.permutation(n)[:500]] = np.array([-1, n, C.I32_MAX, -(1 << 31)], np.int32)[rng.integers(0, 4, 500)]
    bad_pos[[0, 63, 64, n - 1]] = (-1, n, C.I32_MAX, n)
    beyond, jumpy = rp + np.arange(n_users + 1) * 2400, rp.copy()
    jumpy[[2, 5, 7]] = (-50, 1 << 40, I64_MIN)
    for name, h_rp, h_pos in (("descending", rp[::-1].copy(), pos), ("beyond", beyond, pos), ("jumpy", jumpy, bad_pos), ("both", beyond[::-1].copy(), bad_pos)):
        for drop in (np.array([0, 3, 3, n_users - 1, 5], np.int32), NONE):
            status, _, _, _, _, got = run_dedup(sess, T.TrimProblem(name, n_users, items, times, h_rp, h_pos, T0, drop), 50, keep, (n, n))
            assert status == _lib.OK and 0 <= got[1] <= got[0] <= n, (name, got)


def refusal_case(sess, keep):
    """keep outside {1, 2}, n_cols < 1, and the trim's: n_events >= 2^31, too many users, a NULL the call needs, times_ms and out_times not NULL together"""
    t = T.make_word_problem(129, True, "random")
    status = lambda n_cols=1000, keep=keep, t=t, **kw: run_dedup(sess, t, n_cols, keep, (t.n_events, t.n_events), **kw)[0]      # noqa: E731
    assert status() == status(n_cols=1) == status(n_cols=C.I32_MAX) == status(null=("times", "o_times")) == _lib.OK
    assert all(status(keep=k) == _lib.BAD_ARG for k in (0, 3, -1, 1 << 30)) and all(status(n_cols=c) == _lib.BAD_ARG for c in (0, -1, -(1 << 31)))
    assert all(status(null=(name,)) == _lib.BAD_ARG for name in ("s", "items", "times", "rp", "pos", "drop", "o_items", "o_times", "o_rp", "o_pos", "counts"))
    lib, ptr = sess.lib, sess.empty(8, torch.int64).data_ptr()      # the counts are refused before anything is read
    for n, nu, nd in ((1 << 31, 1, 0), (-1, 1, 0), (1, -1, 0), (1, 0x7ffffff1, 0), (1, 1, -1)):
        assert lib.urcco_dev_history_dedup(sess.handle, n, ptr, None, nu, ptr, ptr, 0, nd, ptr, 5, KEEPS[keep], ptr, None, ptr, ptr, ptr) == _lib.BAD_ARG, (n, nu, nd)
    assert lib.urcco_version() == 305


def host_keep(users, items, times, n_users, n_cols, keep, cut=None):
    """bool [n]: the events of a stream that survive the cut and the duplicate rule, from the users array"""
    inside = np.flatnonzero((users >= 0) & (users < n_users))
    order = inside[np.argsort(users[inside], kind="stable")].astype(np.int32)
    t = T.TrimProblem("host", n_users, items, times, row_ptr_ref(users, n_users), order, cut if cut is not None and times is not None else I64_MIN, NONE)
    return (np.ones(users.size, bool) if times is None else times >= t.min_time) & ~dup_ref(t, n_cols, keep)


class DedupHost(L.HostHistory):
    """history_lifecycle_cases' host model with the duplicate rule and D27's cap over the survivors"""

    def dedup(self, keep, n_cols, caps):
        for ev, (u, i, t) in self.streams.items():
            ok = host_keep(u, i, t, self.n_users, n_cols[ev], keep)
            u, i, t = u[ok], i[ok], t[ok] if t is not None else None
            ok = C.host_cap(u, t, self.n_users, caps[ev]) if ev in caps else np.ones(u.size, bool)
            self.streams[ev] = (u[ok], i[ok], t[ok] if t is not None else None)


def python_case(sess, keep):
    """create, dedup, append, dedup + cap on ONE DeviceHistory; after every step the state, the history rows and batch_predict against the host model; the
    matrices before and after a dedup; user_recommendations against from_streams over the host's streams; the ValueErrors, with nothing modified"""
    from universal_recommender_amd.history import DeviceHistory
    rng = np.random.default_rng(101)
    stack = L.stack_for(sess)
    planted = [2 * HD + 4, 300, 65, 64, 63, 1, 0]
    n0 = len(planted) + 300
    some = lambda n: rng.integers(len(planted), n0, n)      # noqa: E731
    steps = [{"purchase": L._events(rng, np.repeat(np.arange(n0), planted + rng.integers(0, 30, 300).tolist()), L.N_ITEMS, (0, 200), negative=4),
              "view": L._events(rng, some(1500), L.N_VIEW, (0, 200))}, {},
             {"purchase": L._events(rng, np.concatenate([some(1500), np.full(100, 0), np.full(70, 2)]), L.N_ITEMS, (100, 300)),
              "wish": L._events(rng, np.concatenate([some(300), np.full(150, 1)]), L.N_ITEMS)}, {"purchase": 20, "wish": 3}]
    h, dh = DedupHost(), None
    sched = L.Schedule(False, [], list(range(len(planted))), n0)
    q_users, col_map = L.query_users(sched), L.view_col_map()
    mats = lambda: [(m.row_ptr.cpu().numpy(), m.col_idx.cpu().numpy()[: int(m.row_ptr[-1])]) for m in dh.matrices(list(dh.types))[2].values()]      # noqa: E731
    for step in steps:
        if "purchase" in step and isinstance(step["purchase"], tuple):
            dev = L._device_batch(sess, step, False)
            dh = DeviceHistory.from_streams(sess, stack[1], dev, n_users=n0) if dh is None else dh.append(dev, n_users=n0)
            h.append(step, n0)
        else:
            before, m_before = {ev: h.n_events(ev) for ev in h.streams}, mats()
            assert dh.trim(remove_duplicates=keep if step else {ev: keep for ev in dh.types}, max_events_per_user=step or None) is dh
            h.dedup(keep, {ev: st.n_cols for ev, st in dh.types.items()}, step)
            assert dh.last_trim == {ev: (before[ev], h.n_events(ev)) for ev in before} and h.n_events("purchase") < before["purchase"], dh.last_trim
            assert step or all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(m_before, mats()))
        if "view" in dh.types and dh.types["view"].col_map is None:
            dh.types["view"].col_map = put(sess, col_map)
        sess.synchronize()
        L.check_state(dh, h)
        L.check_rows(sess, dh, h, q_users, col_map)
        L.check_predict(stack, dh, h, sched)
    whole = DeviceHistory.from_streams(sess, stack[1], C._dev(sess, h.streams), n_users=n0)
    assert all(torch.equal(a, b) for a, b in zip(stack[0].user_recommendations(stack[1], dh), stack[0].user_recommendations(stack[1], whole)))
    for bad in ("newest", 1, True, {"no such event": keep}, {"purchase": "both"}, {"purchase": None}):
        try:
            dh.trim(remove_duplicates=bad)
        except ValueError:
            continue
        raise AssertionError(f"trim(remove_duplicates={bad!r}) did not raise")
    L.check_state(dh, h)      # nothing was modified


def larger_shape_case(sess, keep):
    """2^20 + 77 events over 2^16 users, Zipf(1.3), items Zipf(1.1) over 2^14 columns: users of every class"""
    rng = np.random.default_rng(37)
    n, n_users, n_cols = (1 << 20) + 77, 1 << 16, 1 << 14
    users = ((rng.zipf(1.3, n) - 1) % n_users).astype(np.int32)
    users[rng.integers(0, n, 500)] = -1
    cnt = np.bincount(users[users >= 0], minlength=n_users)
    assert (cnt <= 1).any() and ((cnt > 1) & (cnt <= 64)).any() and ((cnt > 64) & (cnt <= HD)).any() and (cnt > HD).any()
    items, times = ((rng.zipf(1.1, n) - 1) % n_cols).astype(np.int32), (T0 + rng.integers(-1000, 1000, n)).astype(np.int64)
    t = T.TrimProblem("larger shape", n_users, items, times, *T.host_index(users, n_users, rng), T0 - 500, np.array([3, 70000, -1], np.int32))
    assert 0 < np.count_nonzero(check_dedup(sess, t, n_cols, keep)) < n // 2


# (case, arguments behind the session and keep): the five item patterns over every segment length, the time patterns of the cap's cases, the rest
CASES = [(segment_case, (i, "ties")) for i in ("one", "distinct", "twice", "chain", "load")] + [(segment_case, ("twice", tm)) for tm in C.TIME_PATTERNS[1:]] + [
    (f, ()) for f in (column_table_case, index_order_case, no_column_case, time_cut_case, degenerate_case, hostile_case, refusal_case, python_case)]
IDS = [" ".join((f.__name__,) + a) for f, a in CASES]
