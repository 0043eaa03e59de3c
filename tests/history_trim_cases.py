"""urcco_dev_history_trim (decision D22 of DESIGN.md, include/urcco.h): the problems and checks that tests/test_sim_history_trim.py and
tests/test_gpu_history_trim.py share.  The contract, restated in numpy (trim_ref):

    keep[p]    = (times is None or times[p] >= min_time) and no index entry of a listed user names p
    new_of[p]  = the number of kept positions below p;  K = keep.sum()
    out_items, out_times = items[keep], times[keep]
    n_e        = min(row_ptr[n_users], n_events);  ikeep[e] = keep[pos[e]] for e < n_e;  KE = ikeep.sum()
    out_pos    = new_of[pos[:n_e][ikeep]];  out_row_ptr[u] = the number of kept entries below row_ptr[u];  counts = [K, KE]

Every index here is built on the host, in a random order inside every user's segment, and holds exactly n_e entries: a read past them faults under
HIPSIM_GUARD.  run_trim allocates every output at exactly K, KE and n_users + 1 entries (one sentinel entry where that is 0) plus `pad` sentinel
entries, and check_trim asserts that everything behind the result still holds the sentinel."""
import copy
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import history_ref as H
from history_append_cases import put, row_ptr_ref
from universal_recommender_amd import _lib

I64_MIN, I64_MAX = H.I64_MIN, H.I64_MAX
SENTINEL = H.SENTINEL
WORD_SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 4097)
T0 = 1_600_000_000_000


@dataclass
class TrimProblem:
    name: str
    n_users: int
    items: np.ndarray             # int32 [n_events]
    times: Optional[np.ndarray]   # int64 [n_events] or None
    row_ptr: np.ndarray           # int64 [n_users + 1]
    pos: np.ndarray               # int32 [n_e]
    min_time: int
    drop: np.ndarray              # int32

    @property
    def n_events(self):
        return int(self.items.size)


def host_index(users, n_users, rng):
    """(row_ptr, pos) of `users`: ids < 0 or >= n_users are nobody's; a random order inside every segment"""
    p = np.flatnonzero((users >= 0) & (users < n_users))
    p = p[rng.permutation(p.size)]
    p = p[np.argsort(users[p], kind="stable")]
    return row_ptr_ref(users, n_users), p.astype(np.int32)


def trim_ref(t: TrimProblem):
    """(keep, new_of, out_items, out_times | None, out_row_ptr, out_pos, counts) of a well-formed index, all numpy"""
    n = t.n_events
    keep = np.ones(n, bool) if t.times is None else t.times >= t.min_time
    n_e = int(min(t.row_ptr[-1], n))
    for u in np.unique(t.drop[(t.drop >= 0) & (t.drop < t.n_users)]):
        keep[t.pos[t.row_ptr[u]:t.row_ptr[u + 1]]] = False
    new_of = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    ikeep = keep[t.pos[:n_e]]
    rank_i = np.concatenate([[0], np.cumsum(ikeep)]).astype(np.int64)
    out_pos = new_of[t.pos[:n_e][ikeep]].astype(np.int32)
    counts = np.array([keep.sum(), ikeep.sum()], np.int64)
    return keep, new_of, t.items[keep], t.times[keep] if t.times is not None else None, rank_i[t.row_ptr], out_pos, counts


def _without_times(t):
    u = copy.copy(t)
    u.times = None
    return u


def run_trim(sess, t: TrimProblem, sizes=None, pad=0, null_times=False):
    """One urcco_dev_history_trim call through ctypes.  sizes: (K, KE) the outputs are allocated for (default: the restatement's); null_times: the
    stream's times are withheld (and out_times), min_time is passed all the same.  Returns (status, out_items, out_times | None, out_row_ptr, out_pos,
    counts) as numpy arrays, the outputs whole: sentinels included."""
    if sizes is None:
        sizes = trim_ref(_without_times(t) if null_times else t)[6]
    k, ke = int(sizes[0]), int(sizes[1])
    have_times = t.times is not None and not null_times
    outs = [sess.empty(max(k, 1) + pad, torch.int32), sess.empty(max(k, 1) + pad, torch.int64) if have_times else None,
            sess.empty(t.n_users + 1 + pad, torch.int64), sess.empty(max(ke, 1) + pad, torch.int32)]
    for o in outs:
        if o is not None:
            o.fill_(SENTINEL)
    counts = sess.empty(2, torch.int64)
    counts.fill_(SENTINEL)
    d_items = put(sess, t.items)
    d_times = (put(sess, t.times) if t.n_events else sess.empty(1, torch.int64)) if have_times else None     # NULL means "no times", also for a stream of no events
    d_rp, d_drop = put(sess, t.row_ptr), put(sess, t.drop)
    d_pos = put(sess, t.pos) if t.pos.size or not t.n_events else sess.empty(1, torch.int32)      # an index without entries still has an array; no entry of it is read
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None      # noqa: E731 -- an array of no entries is passed as NULL
    status = sess.lib.urcco_dev_history_trim(sess.handle, t.n_events, ptr(d_items), ptr(d_times), t.n_users, d_rp.data_ptr(), ptr(d_pos), t.min_time, t.drop.size,
                                             ptr(d_drop), outs[0].data_ptr(), outs[1].data_ptr() if have_times else None, outs[2].data_ptr(), outs[3].data_ptr(),
                                             counts.data_ptr())
    sess.synchronize()
    return (status,) + tuple(o.cpu().numpy() if o is not None else None for o in outs) + (counts.cpu().numpy(),)


def check_trim(sess, t: TrimProblem, pad=0, null_times=False):
    """The call against the restatement: the five outputs, and the sentinel in every entry behind them.  Returns (K, KE)."""
    ref = _without_times(t) if null_times else t
    keep, new_of, w_items, w_times, w_rp, w_pos, w_counts = trim_ref(ref)
    status, items, times, rp, pos, counts = run_trim(sess, t, w_counts, pad, null_times)
    assert status == _lib.OK, t.name
    k, ke = int(w_counts[0]), int(w_counts[1])
    assert np.array_equal(counts, w_counts), (t.name, counts, w_counts)
    assert np.array_equal(items[:k], w_items), t.name
    assert (times is None) == (w_times is None) and (times is None or np.array_equal(times[:k], w_times)), t.name
    assert np.array_equal(rp[: t.n_users + 1], w_rp), t.name
    assert np.array_equal(pos[:ke], w_pos), t.name
    assert (items[k:] == SENTINEL).all() and (times is None or (times[k:] == SENTINEL).all()), f"{t.name}: written at or past out_items / out_times[K]"
    assert (pos[ke:] == SENTINEL).all() and (rp[t.n_users + 1:] == SENTINEL).all(), f"{t.name}: written at or past out_pos[KE] / out_row_ptr[n_users + 1]"
    assert items.size == max(k, 1) + pad and pos.size == max(ke, 1) + pad and rp.size == t.n_users + 1 + pad
    return k, ke


# ---- word edges -----------------------------------------------------------------------------------------------------------------------------------
WORD_PATTERNS = ("words", "random", "nothing", "everything")


def make_word_problem(n, nobody, pattern, seed=3):
    """n events over 9 users of which the first two, the last two and users 4, 5 own nothing.  nobody: some positions belong to nobody -- the first,
    the middle and the last one among them, as many as make n_e a multiple of 64 (n >= 67; three otherwise).  pattern, by the time
    rule and one dropped user: "words" -- word 0 kept entirely, word 1 dropped entirely, word 2 alternating, the rest at random; "random";
    "nothing" dropped (the outputs are the inputs); "everything" dropped (K == 0)."""
    rng = np.random.default_rng(seed + n)
    n_users = 9
    users = rng.choice(np.array([2, 3, 6], np.int32), n)
    if nobody and n:
        n_e = (n - 3) // 64 * 64 if n >= 67 else max(n - 3, 0)
        free = np.setdiff1d(np.arange(n), [0, n // 2, n - 1])
        who = np.concatenate([np.unique([0, n // 2, n - 1]), free[rng.permutation(free.size)]])[: n - n_e]
        users[who] = -1
    cut = T0
    times = cut + rng.integers(0, 5, n)
    drop = np.zeros(0, np.int32)
    if pattern in ("words", "random"):
        old = rng.random(n) < 0.4
        if pattern == "words":
            old[:64], old[64:128], old[128:192] = False, True, (np.arange(128, 192) % 2 == 1)[: max(min(n, 192) - 128, 0)]
            for w in (users[:64], users[128:192]):       # user 3 is dropped: none of its events in the word kept entirely and in the alternating one
                w[w == 3] = 2
        times[old] = cut - 1 - rng.integers(0, 5, int(old.sum()))
        drop = np.array([3], np.int32)
    elif pattern == "everything":
        times[:] = cut - 1
    rp, pos = host_index(users, n_users, rng)
    items = rng.integers(-1, 1000, n).astype(np.int32)
    return TrimProblem(f"n={n} nobody={nobody} {pattern}", n_users, items, times.astype(np.int64), rp, pos, cut, drop)


def assert_word_problem(t: TrimProblem, n, nobody, pattern):
    """From the problem alone: what make_word_problem promises"""
    keep, _, _, _, _, _, counts = trim_ref(t)
    n_e = int(t.row_ptr[-1])
    assert t.n_events == n and t.pos.size == n_e
    if nobody and n:
        named = np.zeros(n, bool)
        named[t.pos] = True
        assert n_e < n and not named[0] and not named[n // 2] and not named[n - 1]
        assert n < 67 or (n_e % 64 == 0 and n_e > 0)                     # rank(n_e) must not read a word past the bitmap
    else:
        assert n_e == n
    if pattern == "words" and n >= 192:
        assert keep[:64].all() and not keep[64:128].any() and np.array_equal(keep[128:192], np.arange(128, 192) % 2 == 0)
    if pattern == "nothing":
        assert keep.all() and counts[0] == n and counts[1] == n_e
    if pattern == "everything":
        assert counts[0] == 0 and counts[1] == 0


def word_cases(sess):
    for n in WORD_SIZES:
        for nobody in (False, True):
            for pattern in WORD_PATTERNS:
                t = make_word_problem(n, nobody, pattern)
                assert_word_problem(t, n, nobody, pattern)
                k, ke = check_trim(sess, t)
                if pattern == "nothing":       # the outputs equal the inputs
                    _, items, times, rp, pos, _ = run_trim(sess, t)
                    assert np.array_equal(items[:k], t.items) and np.array_equal(times[:k], t.times) and np.array_equal(rp, t.row_ptr) and np.array_equal(pos[:ke], t.pos)
    for n in (129, 4097):                      # padded buffers: the padding is untouched
        for pattern in ("words", "everything"):
            check_trim(sess, make_word_problem(n, True, pattern), pad=70)


# ---- the time rule --------------------------------------------------------------------------------------------------------------------------------
def time_cases(sess):
    rng = np.random.default_rng(17)
    n, n_users = 300, 6
    users = rng.integers(0, n_users, n).astype(np.int32)
    rp, pos = host_index(users, n_users, rng)
    items = rng.integers(0, 50, n).astype(np.int32)
    none = np.zeros(0, np.int32)
    for cut in (T0, -5, 0, I64_MIN + 1, I64_MAX):
        lo, hi = max(cut - 1, I64_MIN), min(cut + 1, I64_MAX)
        times = np.array([cut, lo, hi, -1, -(1 << 40), I64_MIN, I64_MAX, 0], np.int64)[rng.integers(0, 8, n)]
        times[:3] = (cut, lo, hi)
        t = TrimProblem(f"cut={cut}", n_users, items, times, rp, pos, cut, none)
        keep = trim_ref(t)[0]
        assert keep[0] and not keep[1]                                   # equal to the cut-off: kept; one below: dropped
        assert (times < 0).any()
        check_trim(sess, t)
    times = np.array([I64_MIN, -1, 0, I64_MAX], np.int64)[rng.integers(0, 4, n)]
    k, _ = check_trim(sess, TrimProblem("INT64_MIN", n_users, items, times, rp, pos, I64_MIN, none))
    assert k == n                                                        # INT64_MIN keeps everything
    k, _ = check_trim(sess, TrimProblem("INT64_MAX", n_users, items, times, rp, pos, I64_MAX, none))
    assert 0 < k == np.count_nonzero(times == I64_MAX) < n
    # times_ms == NULL: the time rule is ignored whatever min_time_ms says
    for cut in (T0, I64_MAX):
        k, ke = check_trim(sess, TrimProblem(f"no times, cut={cut}", n_users, items, np.full(n, T0 - 7, np.int64), rp, pos, cut, np.array([1], np.int32)), null_times=True)
        assert k == ke == n - (rp[2] - rp[1])


# ---- users ----------------------------------------------------------------------------------------------------------------------------------------
BIG_USER = 70000     # more entries than HT_SPLIT * HT_CHUNK = 65536: its blocks take a second round of chunks


def make_user_problem(seed=13, big=5000):
    """Users: runs of empty ones at both ends and in the middle, one-event users, users of 63 / 64 / 65 events, one of `big` entries (> 4096), one whose
    whole segment is older than the cut-off.  Some positions are nobody's."""
    rng = np.random.default_rng(seed)
    counts = [0, 0, 0, 1, 1, big, 0, 0, 1, 63, 64, 65, 0, 40, 1, 300, 0, 0]
    named = {"first": 3, "big": 5, "old": 13, "last": 15, "empty": 7}
    n_users = len(counts)
    users = np.concatenate([np.repeat(np.arange(n_users, dtype=np.int32), counts), np.full(11, -1, np.int32)])
    users = users[rng.permutation(users.size)]
    times = (T0 + rng.integers(-20, 20, users.size)).astype(np.int64)
    times[users == named["old"]] = T0 - 100
    rp, pos = host_index(users, n_users, rng)
    items = rng.integers(-1, 1000, users.size).astype(np.int32)
    return TrimProblem("users", n_users, items, times, rp, pos, T0, np.zeros(0, np.int32)), named


def user_cases(sess, big=5000):
    t, named = make_user_problem(big=big)
    cnt = np.diff(t.row_ptr)
    assert cnt[:3].sum() == 0 and cnt[-2:].sum() == 0 and cnt[6:8].sum() == 0 and cnt[named["big"]] == big > 4096 and (cnt == 1).sum() >= 4
    assert cnt[named["first"]] > 0 and not cnt[: named["first"]].any() and cnt[named["last"]] > 0 and not cnt[named["last"] + 1:].any()
    keep = trim_ref(t)[0]
    assert not keep[t.pos[t.row_ptr[named["old"]]:t.row_ptr[named["old"] + 1]]].any()      # a whole segment dropped by time
    nu = t.n_users
    lists = {"nobody": [], "hostile ids": [named["big"], -1, nu, named["empty"], named["big"], nu + 5, -(1 << 31), named["big"]],
             "first": [named["first"]], "last": [named["last"]], "first and last": [named["last"], named["first"]], "all": list(range(nu))[::-1],
             "only ids outside": [-1, nu], "ones": [3, 4, 8, 14]}
    for name, ids in lists.items():
        for min_time in (T0, I64_MIN):
            u = copy.copy(t)
            u.name, u.drop, u.min_time = f"drop {name} min_time {min_time}", np.array(ids, np.int32), min_time
            k, ke = check_trim(sess, u)
            if name == "all":
                assert ke == 0 and (k == 11 if min_time == I64_MIN else 0 < k <= 11)        # nobody's events stay: the time rule alone decides
    u = copy.copy(t)
    u.name, u.drop = "padded", np.array([named["big"], named["first"], 9], np.int32)
    check_trim(sess, u, pad=130)


# ---- a hostile index ------------------------------------------------------------------------------------------------------------------------------
def hostile_cases(sess):
    """Whatever idx_row_ptr and idx_pos hold: URCCO_OK, the run ends, no access leaves the arrays (HIPSIM_GUARD).  Values: 0 <= KE <= K <= n_events."""
    rng = np.random.default_rng(19)
    n, n_users = 1000, 12
    users = rng.integers(0, n_users, n).astype(np.int32)
    rp, pos = host_index(users, n_users, rng)
    items = rng.integers(0, 50, n).astype(np.int32)
    times = (T0 + rng.integers(-20, 20, n)).astype(np.int64)
    bad_pos = pos.copy()
    bad_pos[rng.permutation(n)[:90]] = np.array([-1, n, (1 << 31) - 1], np.int32)[rng.integers(0, 3, 90)]
    bad_pos[[0, 63, 64, n - 1]] = (-1, n, (1 << 31) - 1, n)
    descending = rp[::-1].copy()
    beyond = rp + np.arange(n_users + 1) * 400                       # exceeds n_events from the fourth user on; the last is 1000 + 4800
    jumpy = rp.copy()
    jumpy[[2, 5, 7]] = (-50, 1 << 40, I64_MIN)
    drop = np.array([0, 3, 3, n_users - 1, 5], np.int32)
    for name, h_rp, h_pos in (("pos", rp, bad_pos), ("descending", descending, pos), ("beyond", beyond, pos), ("jumpy", jumpy, bad_pos), ("both", beyond[::-1].copy(), bad_pos)):
        for d in (drop, np.zeros(0, np.int32)):
            t = TrimProblem(f"hostile {name}", n_users, items, times, h_rp, h_pos, T0, d)
            status, _, _, _, _, counts = run_trim(sess, t, sizes=(n, n))
            assert status == _lib.OK and 0 <= counts[1] <= counts[0] <= n, (name, counts)


# ---- rows over a trimmed history ------------------------------------------------------------------------------------------------------------------
ROW_CAPS = (5, 64, 5000)      # below, at and above users' event counts (planted: 63, 64, 65, 4095 .. 10000)


def trimmed_problem(sess, p: H.Problem, cut, drop):
    """(the filtered problem, its DeviceProblem, a DeviceProblem of p whose streams and indexes went through history_trim instead).  The filtered
    streams are what the contract keeps: per stream the events that pass the time rule and are not a dropped user's."""
    drop = np.asarray(drop, np.int32)
    d_drop = put(sess, drop)
    full = H.DeviceProblem(sess, p)
    f = copy.copy(p)
    f.streams = []
    ev = []
    for s, (n_cols, rp, pos, items, times, cmap) in zip(p.streams, full.ev):
        keep = ~np.isin(s.users, drop) & ((s.times >= cut) if s.times is not None else True)
        f.streams.append(H.Stream(s.n_cols, s.users[keep], s.items[keep], s.times[keep] if s.times is not None else None, s.col_map, s.blacklist))
        o_items, o_times, o_rp, o_pos, counts = sess.history_trim(s.users.size, items, times, rp, pos, cut, d_drop)
        sess.synchronize()
        k, ke = (int(x) for x in counts.cpu())
        assert k == int(keep.sum()) and ke == int((f.streams[-1].users >= 0).sum())
        assert np.array_equal(o_items[:k].cpu().numpy(), s.items[keep]) and (o_times is None or np.array_equal(o_times[:k].cpu().numpy(), s.times[keep]))
        ev.append((n_cols, o_rp, o_pos[: max(ke, 1)], o_items[: max(k, 1)], o_times[: max(k, 1)] if o_times is not None else None, cmap))
    filtered = H.DeviceProblem(sess, f)
    trimmed = copy.copy(filtered)
    trimmed.ev = ev
    return f, filtered, trimmed


def rows_case(sess):
    """history_rows over a trimmed history == over history_index of the filtered streams == the restatement, bit for bit: term rows with caps below,
    at and above the users' counts, and exclusion rows, on history_ref's problem.  The cut-off drops about half of the timed events; the heavy user,
    a user of 64 events and an unknown id are dropped."""
    p = H.make_problem()
    cnt0 = np.bincount(p.streams[0].users[p.streams[0].users >= 0], minlength=p.n_users)
    drop = [int(np.argmax(cnt0)), int(np.flatnonzero(cnt0 == 64)[0]), p.n_users + 3, int(np.argmax(cnt0))]
    f, filtered, trimmed = trimmed_problem(sess, p, T0 + 25, drop)
    after = np.bincount(f.streams[0].users[f.streams[0].users >= 0], minlength=p.n_users)
    assert after[drop[0]] == 0 and after.max() > 64 and 0 < after.sum() < cnt0.sum() * 3 // 4 and f.streams[1].users.size < p.streams[1].users.size
    assert any((after < c).any() and (after > c).any() for c in ROW_CAPS)
    for cap in ROW_CAPS:
        _, terms_a, excl_a = H.check(filtered, [cap] * 3)
        _, terms_b, excl_b = H.check(trimmed, [cap] * 3)
        for ra, rb in zip(terms_a + [excl_a], terms_b + [excl_b]):
            assert all(np.array_equal(x, y) for x, y in zip(ra, rb))


def chain_case(sess):
    """trim, history_append, trim again: the stream and the index are those of the whole stream filtered by what each trim saw"""
    rng = np.random.default_rng(23)
    n, n_users, cut_at = 3000, 40, 1900
    users = ((rng.zipf(1.5, n) - 1) % n_users).astype(np.int32)
    users[rng.random(n) < 0.02] = -1
    times = (T0 + rng.integers(0, 100, n)).astype(np.int64)
    items = rng.integers(0, 500, n).astype(np.int32)
    c1, c2, drop1, drop2 = T0 + 30, T0 + 55, np.array([0, 7], np.int32), np.array([1, 7, 39], np.int32)
    rp, pos = host_index(users[:cut_at], n_users, rng)
    a_items, a_times, a_rp, a_pos, counts = sess.history_trim(cut_at, put(sess, items[:cut_at]), put(sess, times[:cut_at]), put(sess, rp), put(sess, pos), c1, put(sess, drop1))
    sess.synchronize()
    k1 = int(counts[0])
    keep1 = (times[:cut_at] >= c1) & ~np.isin(users[:cut_at], drop1)
    assert k1 == keep1.sum()
    b_rp, b_pos = sess.history_append(a_rp, a_pos[:k1], k1, put(sess, users[cut_at:]), n_users)
    m = k1 + n - cut_at
    b_items, b_times = sess.empty(m, torch.int32), sess.empty(m, torch.int64)
    b_items[:k1].copy_(a_items[:k1]), b_items[k1:].copy_(torch.from_numpy(items[cut_at:]))
    b_times[:k1].copy_(a_times[:k1]), b_times[k1:].copy_(torch.from_numpy(times[cut_at:]))
    c_items, c_times, c_rp, c_pos, counts = sess.history_trim(m, b_items, b_times, b_rp, b_pos, c2, put(sess, drop2))
    sess.synchronize()
    keep = (times >= c2) & ~np.isin(users, drop2)
    keep[:cut_at] &= keep1
    k, ke = (int(x) for x in counts.cpu())
    w_users = users[keep]
    assert k == keep.sum() and ke == (w_users >= 0).sum() and 0 < ke < k < m
    assert np.array_equal(c_items[:k].cpu().numpy(), items[keep]) and np.array_equal(c_times[:k].cpu().numpy(), times[keep])
    h_rp, h_pos = c_rp.cpu().numpy(), c_pos[:ke].cpu().numpy()
    assert np.array_equal(h_rp, row_ptr_ref(w_users, n_users))
    for u in range(n_users):
        assert np.array_equal(np.sort(h_pos[h_rp[u]:h_rp[u + 1]]), np.flatnonzero(w_users == u)), u


# ---- bad arguments --------------------------------------------------------------------------------------------------------------------------------
def bad_argument_cases(sess):
    lib = sess.lib
    t = make_word_problem(129, True, "random")
    n, nu = t.n_events, t.n_users
    d = dict(items=put(sess, t.items), times=put(sess, t.times), rp=put(sess, t.row_ptr), pos=put(sess, t.pos), drop=put(sess, t.drop),
             o_items=sess.empty(n, torch.int32), o_times=sess.empty(n, torch.int64), o_rp=sess.empty(nu + 1, torch.int64), o_pos=sess.empty(n, torch.int32),
             counts=sess.empty(2, torch.int64))
    ok = dict(s=sess.handle, n=n, nu=nu, min_time=t.min_time, n_drop=t.drop.size, **{k: v.data_ptr() for k, v in d.items()})

    def call(**kw):
        a = dict(ok, **kw)
        return lib.urcco_dev_history_trim(a["s"], a["n"], a["items"], a["times"], a["nu"], a["rp"], a["pos"], a["min_time"], a["n_drop"], a["drop"], a["o_items"],
                                          a["o_times"], a["o_rp"], a["o_pos"], a["counts"])

    assert call() == _lib.OK
    assert call(n=1 << 31) == _lib.BAD_ARG and call(n=1 << 62) == _lib.BAD_ARG      # n_events >= 2^31
    for name in ("n", "nu", "n_drop"):                                               # a negative count
        assert call(**{name: -1}) == _lib.BAD_ARG, name
    assert call(nu=0x7ffffff1) == _lib.BAD_ARG
    for name in ("s", "items", "rp", "pos", "drop", "o_items", "o_rp", "o_pos", "counts"):      # a NULL the call needs
        assert call(**{name: None}) == _lib.BAD_ARG, name
    assert call(times=None) == _lib.BAD_ARG and call(o_times=None) == _lib.BAD_ARG   # out_times and times_ms: NULL together or not at all
    # NULLs the call does not need
    assert call(times=None, o_times=None) == _lib.OK
    assert call(n_drop=0, drop=None) == _lib.OK
    assert call(nu=0, rp=None, n_drop=0, drop=None) == _lib.OK                       # no users: every event is nobody's, the time rule alone
    sess.synchronize()
    assert int(d["o_rp"][0]) == 0 and int(d["counts"][1]) == 0 and int(d["counts"][0]) == np.count_nonzero(t.times >= t.min_time)
    assert call(n=0, items=None, pos=None, o_items=None, o_pos=None) == _lib.OK
    assert call(n=0, items=None, times=None, nu=0, rp=None, pos=None, n_drop=0, drop=None, o_items=None, o_times=None, o_pos=None) == _lib.OK
    sess.synchronize()
    assert int(d["o_rp"][0]) == 0 and d["counts"].tolist() == [0, 0]
    assert lib.urcco_version() == 305
