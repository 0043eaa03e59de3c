"""urcco_dev_history_cap (decision D27 of DESIGN.md, include/urcco.h): the problems and checks that tests/test_sim_history_cap.py and
tests/test_gpu_history_cap.py share.  The contract, restated in numpy (cap_ref): the trim's restatement (history_trim_cases.trim_ref) with one more rule,

    valid(u)   = the entries e of u's clamped segment with 0 <= pos[e] < n_events
    key(e)     = (times[pos[e]] ^ sign bit as uint64, pos[e]), pos[e] alone without times
    capped[p]  = an entry of some user u names p and its key is not among the max_per_user largest keys of valid(u)
    keep[p]    = passes the time rule and no entry of a listed user names p and not capped[p]

Every output buffer has exactly the size the restatement gives (history_trim_cases.run_trim's rule), so the rerun under HIPSIM_GUARD faults on a write
past the results and on a read past the index entries.  The Python level: DeviceHistory.trim(max_events_per_user=...) against from_streams over streams
filtered on the host, and a schedule on one object against history_lifecycle_cases' host model extended by the cap rule."""
import copy

import numpy as np
import torch

import history_lifecycle_cases as L
import history_ref as H
import history_trim_cases as T
from history_append_cases import put, row_ptr_ref
from universal_recommender_amd import _lib

I64_MIN, I64_MAX = H.I64_MIN, H.I64_MAX
I32_MAX = (1 << 31) - 1
SENTINEL = T.SENTINEL
T0 = T.T0
SIGN = np.uint64(1 << 63)
CAPS = (1, 2, 63, 64, 65, 500, 4096, 5000)
TIME_PATTERNS = ("ties", "equal", "top byte", "low byte", "none", "extremes")
BIG_OWNER = (100_000, 100_100)      # one user owns the first of the second


def segment_lengths(cap):
    return sorted({0, 1, cap - 1, cap, cap + 1, 63, 64, 65, 4095, 4096, 4097, 8193})


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------
def capped_ref(n_events, times, n_users, row_ptr, pos, cap):
    """bool [n_events]: the positions the cap rule drops"""
    out = np.zeros(n_events, bool)
    if n_users == 0:
        return out
    n_e = int(min(max(int(row_ptr[-1]), 0), n_events))
    rp = np.clip(row_ptr.astype(object), 0, n_e).astype(np.int64)      # object: row starts beyond int64's comfortable range clamp as integers
    for u in np.flatnonzero(rp[1:] - rp[:-1] > cap):
        seg = pos[rp[u]:rp[u + 1]].astype(np.int64)
        seg = seg[(seg >= 0) & (seg < n_events)]
        if seg.size <= cap:
            continue
        tk = times[seg].view(np.uint64) ^ SIGN if times is not None else np.zeros(seg.size, np.uint64)
        order = np.lexsort((seg, tk))                                  # ascending by (time, position)
        out[seg[order[: seg.size - cap]]] = True
    return out


def cap_ref(t: T.TrimProblem, cap):
    """(keep, out_items, out_times | None, out_row_ptr, out_pos, counts) of a well-formed index: trim_ref with the cap rule"""
    n = t.n_events
    keep = np.ones(n, bool) if t.times is None else t.times >= t.min_time
    n_e = int(min(t.row_ptr[-1], n)) if t.n_users else 0
    for u in np.unique(t.drop[(t.drop >= 0) & (t.drop < t.n_users)]):
        keep[t.pos[t.row_ptr[u]:t.row_ptr[u + 1]]] = False
    if cap is not None:
        keep &= ~capped_ref(n, t.times, t.n_users, t.row_ptr, t.pos, cap)
    new_of = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    ikeep = keep[t.pos[:n_e]]
    rank_i = np.concatenate([[0], np.cumsum(ikeep)]).astype(np.int64)
    out_pos = new_of[t.pos[:n_e][ikeep]].astype(np.int32)
    counts = np.array([keep.sum(), ikeep.sum()], np.int64)
    w_rp = rank_i[t.row_ptr] if t.n_users else np.zeros(1, np.int64)
    return keep, t.items[keep], t.times[keep] if t.times is not None else None, w_rp, out_pos, counts


def run_cap(sess, t: T.TrimProblem, cap, sizes, pad=0):
    """One urcco_dev_history_cap call through ctypes (cap None: urcco_dev_history_trim, for the comparison), the outputs allocated at sizes = (K, KE)
    entries (one where that is 0) plus `pad`, all filled with the sentinel.  Returns (status, out_items, out_times | None, out_row_ptr, out_pos, counts),
    the outputs whole."""
    k, ke = int(sizes[0]), int(sizes[1])
    have_times = t.times is not None
    outs = [sess.empty(max(k, 1) + pad, torch.int32), sess.empty(max(k, 1) + pad, torch.int64) if have_times else None,
            sess.empty(t.n_users + 1 + pad, torch.int64), sess.empty(max(ke, 1) + pad, torch.int32)]
    for o in outs:
        if o is not None:
            o.fill_(SENTINEL)
    counts = sess.empty(2, torch.int64)
    counts.fill_(SENTINEL)
    d_items = put(sess, t.items)
    d_times = (put(sess, t.times) if t.n_events else sess.empty(1, torch.int64)) if have_times else None
    d_rp, d_drop = put(sess, t.row_ptr), put(sess, t.drop)
    d_pos = put(sess, t.pos) if t.pos.size or not t.n_events else sess.empty(1, torch.int32)
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None      # noqa: E731 -- an array of no entries is passed as NULL
    head = (sess.handle, t.n_events, ptr(d_items), ptr(d_times), t.n_users, ptr(d_rp) if t.n_users else None, ptr(d_pos), t.min_time, t.drop.size, ptr(d_drop))
    tail = (outs[0].data_ptr(), outs[1].data_ptr() if have_times else None, outs[2].data_ptr(), outs[3].data_ptr(), counts.data_ptr())
    if cap is None:
        status = sess.lib.urcco_dev_history_trim(*head, *tail)
    else:
        status = sess.lib.urcco_dev_history_cap(*head, cap, *tail)
    sess.synchronize()
    return (status,) + tuple(o.cpu().numpy() if o is not None else None for o in outs) + (counts.cpu().numpy(),)


def check_cap(sess, t: T.TrimProblem, cap, pad=0):
    """The call against the restatement: the five outputs, and the sentinel in every entry behind them.  Returns (keep, K, KE)."""
    keep, w_items, w_times, w_rp, w_pos, w_counts = cap_ref(t, cap)
    status, items, times, rp, pos, counts = run_cap(sess, t, cap, w_counts, pad)
    name = f"{t.name} cap={cap}"
    assert status == _lib.OK, name
    k, ke = int(w_counts[0]), int(w_counts[1])
    assert np.array_equal(counts, w_counts), (name, counts, w_counts)
    assert np.array_equal(items[:k], w_items), name
    assert (times is None) == (w_times is None) and (times is None or np.array_equal(times[:k], w_times)), name
    assert np.array_equal(rp[: t.n_users + 1], w_rp), name
    assert np.array_equal(pos[:ke], w_pos), name
    assert (items[k:] == SENTINEL).all() and (times is None or (times[k:] == SENTINEL).all()), f"{name}: written at or past out_items / out_times[K]"
    assert (pos[ke:] == SENTINEL).all() and (rp[t.n_users + 1:] == SENTINEL).all(), f"{name}: written at or past out_pos[KE] / out_row_ptr[n_users + 1]"
    assert items.size == max(k, 1) + pad and pos.size == max(ke, 1) + pad and rp.size == t.n_users + 1 + pad
    return keep, k, ke


# ---- problems -------------------------------------------------------------------------------------------------------------------------------------
def make_times(rng, n, pattern):
    """ties: few distinct values; equal: one value, the position alone decides; top byte / low byte: values that differ in that byte of the key alone
    (the digits sel_differ skips are all the others); extremes: INT64_MIN, -1, 0, INT64_MAX; none: no times"""
    if pattern == "none":
        return None
    if pattern == "ties":
        t = T0 + rng.integers(-6, 6, n)
    elif pattern == "equal":
        t = np.full(n, T0)
    elif pattern == "top byte":
        t = (rng.integers(-128, 128, n) << 56) + 0x0000123456789abc
    elif pattern == "low byte":
        t = T0 // 256 * 256 + rng.integers(0, 256, n)
    else:
        t = np.array([I64_MIN, -1, 0, I64_MAX], np.int64)[rng.integers(0, 4, n)]
    return t.astype(np.int64)


def make_problem(counts, pattern, seed, nobody=5, min_time=I64_MIN, drop=()):
    """users of the given event counts in a shuffled stream, `nobody` positions of no user, a random order inside every index segment"""
    rng = np.random.default_rng(seed)
    n_users = len(counts)
    users = np.concatenate([np.repeat(np.arange(n_users, dtype=np.int32), counts), np.full(nobody, -1, np.int32)])
    users = users[rng.permutation(users.size)]
    rp, pos = T.host_index(users, n_users, rng)
    items = rng.integers(-1, 1000, users.size).astype(np.int32)
    return T.TrimProblem(f"{pattern} {seed}", n_users, items, make_times(rng, users.size, pattern), rp, pos, min_time, np.array(drop, np.int32)), users


def assert_classes(t, cap, want):
    """from the problem alone: which of the mark's classes its users reach -- nothing (m <= cap), wave (<= 64), block (<= 4096), global"""
    m = np.diff(t.row_ptr)
    got = {"nothing": (m <= cap).any(), "wave": ((m > cap) & (m <= 64)).any(), "block": ((m > max(cap, 64)) & (m <= 4096)).any(), "global": ((m > max(cap, 4096))).any()}
    assert all(got[c] for c in want), (t.name, cap, got)


# ---- segment lengths x caps x times ---------------------------------------------------------------------------------------------------------------
def segment_cases(sess, caps=CAPS, patterns=("ties",)):
    for cap in caps:
        lens = segment_lengths(cap)
        for pattern in patterns:
            t, _ = make_problem([0] + lens + [0, 3], pattern, 100 + cap)
            assert_classes(t, cap, ["nothing", "global"] + (["wave"] if cap < 64 else []) + (["block"] if cap < 4096 else []))
            keep, k, ke = check_cap(sess, t, cap)
            kept_of = np.diff(cap_ref(t, cap)[3])
            assert np.array_equal(kept_of, np.minimum(np.diff(t.row_ptr), cap)), (cap, pattern)      # every user keeps min(m, cap)
            if pattern == "equal" or pattern == "none":                 # the position alone decides: a user keeps its LAST positions
                for u in np.flatnonzero(np.diff(t.row_ptr) > cap)[:3]:
                    seg = np.sort(t.pos[t.row_ptr[u]:t.row_ptr[u + 1]])
                    assert keep[seg[-cap:]].all() and not keep[seg[:-cap]].any()


def time_cases(sess):
    segment_cases(sess, caps=(1, 65, 4096), patterns=TIME_PATTERNS[1:])


def big_owner_case(sess, caps=(500, 5000)):
    """one user owns 100 000 of 100 100 events"""
    big, n = BIG_OWNER
    for cap, pattern in zip(caps, ("ties", "low byte")):
        t, _ = make_problem([3, big, 0, n - big - 3 - 5], pattern, 7 + cap)
        assert t.n_events == n and np.diff(t.row_ptr)[1] == big
        _, k, ke = check_cap(sess, t, cap)
        assert ke == 3 + cap + min(cap, n - big - 8) and k == ke + 5


# ---- the order inside a segment -------------------------------------------------------------------------------------------------------------------
def index_order_case(sess):
    """the same stream under three indexes that differ in the order inside the segments (random, ascending, descending): the same kept events"""
    t, users = make_problem([70, 5, 64, 65, 700, 4200, 1], "ties", 41)
    asc = np.flatnonzero(users >= 0)
    asc = asc[np.argsort(users[asc], kind="stable")].astype(np.int32)
    desc = asc.copy()
    for u in range(t.n_users):
        desc[t.row_ptr[u]:t.row_ptr[u + 1]] = desc[t.row_ptr[u]:t.row_ptr[u + 1]][::-1]
    for cap in (2, 64, 500):
        kept = []
        for name, p in (("random", t.pos), ("ascending", asc), ("descending", desc)):
            v = copy.copy(t)
            v.name, v.pos = f"index order {name}", p
            kept.append(check_cap(sess, v, cap)[0])
        assert np.array_equal(kept[0], kept[1]) and np.array_equal(kept[0], kept[2]) and not kept[0].all()


# ---- no cap ---------------------------------------------------------------------------------------------------------------------------------------
def no_cap_cases(sess):
    """a cap at or above every segment, and INT32_MAX: bit-identical to urcco_dev_history_trim, sentinels and all"""
    t, _ = T.make_user_problem()
    t.drop = np.array([3, 9, -1], np.int32)
    top = int(np.diff(t.row_ptr).max())
    sizes = T.trim_ref(t)[6]
    want = run_cap(sess, t, None, sizes, pad=9)
    for cap in (top, top + 1, I32_MAX):
        got = run_cap(sess, t, cap, sizes, pad=9)
        assert got[0] == want[0] == _lib.OK
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(got[1:], want[1:])), cap
    t.min_time = I64_MIN                                                # one less and the cap bites (its victim is the user's oldest event: no time rule here)
    assert cap_ref(t, top - 1)[5][0] == T.trim_ref(t)[6][0] - 1
    check_cap(sess, t, top - 1)


# ---- rule independence ----------------------------------------------------------------------------------------------------------------------------
def independence_case(sess):
    """the cap with min_time_ms and drop_users in one call == the cap alone then the other two == the other two then the cap alone"""
    t, _ = make_problem([0, 70, 64, 65, 700, 4200, 30, 1, 5000], "ties", 53, min_time=T0, drop=(4, 6, 99))
    d = dict(items=put(sess, t.items), times=put(sess, t.times), rp=put(sess, t.row_ptr), pos=put(sess, t.pos), drop=put(sess, t.drop))
    for cap in (1, 40, 64, 600):
        keep, k, ke = check_cap(sess, t, cap)
        by_time, by_cap = t.times >= t.min_time, ~capped_ref(t.n_events, t.times, t.n_users, t.row_ptr, t.pos, cap)
        assert (by_time & ~by_cap).any() and (~by_time & by_cap).any() and 0 < k < t.n_events
        one = sess.history_cap(t.n_events, d["items"], d["times"], d["rp"], d["pos"], cap, t.min_time, d["drop"])
        a = sess.history_cap(t.n_events, d["items"], d["times"], d["rp"], d["pos"], cap)
        sess.synchronize()
        ka = int(a[4][0])
        a = sess.history_trim(ka, a[0], a[1], a[2], a[3], t.min_time, d["drop"])
        b = sess.history_trim(t.n_events, d["items"], d["times"], d["rp"], d["pos"], t.min_time, d["drop"])
        sess.synchronize()
        kb = int(b[4][0])
        b = sess.history_cap(kb, b[0], b[1], b[2], b[3], cap)
        sess.synchronize()
        for x in (a, b):
            assert x[4].tolist() == one[4].tolist() == [k, ke], (cap, x[4].tolist(), one[4].tolist())
            assert torch.equal(x[0][:k], one[0][:k]) and torch.equal(x[1][:k], one[1][:k]) and torch.equal(x[2], one[2]) and torch.equal(x[3][:ke], one[3][:ke]), cap


# ---- degenerate and hostile input -----------------------------------------------------------------------------------------------------------------
def degenerate_cases(sess):
    rng = np.random.default_rng(61)
    none = np.zeros(0, np.int32)
    n = 200
    items, times = rng.integers(0, 50, n).astype(np.int32), (T0 + rng.integers(-5, 5, n)).astype(np.int64)
    # no users: every event is nobody's, the time rule alone
    t = T.TrimProblem("no users", 0, items, times, np.zeros(1, np.int64), none, T0, none)
    keep, k, ke = check_cap(sess, t, 1)
    assert ke == 0 and k == np.count_nonzero(times >= T0)
    # no events
    check_cap(sess, T.TrimProblem("no events", 4, none, np.zeros(0, np.int64), np.zeros(5, np.int64), none, T0, np.array([1], np.int32)), 1)
    check_cap(sess, T.TrimProblem("nothing at all", 0, none, None, np.zeros(1, np.int64), none, T0, none), 3)
    # most positions are nobody's: they stay whatever the cap
    users = np.full(n, -1, np.int32)
    users[rng.permutation(n)[:40]] = 2
    rp, pos = T.host_index(users, 5, rng)
    keep, k, ke = check_cap(sess, T.TrimProblem("nobody's", 5, items, times, rp, pos, I64_MIN, none), 7)
    assert keep[users < 0].all() and ke == 7 and k == n - 33


def hostile_cases(sess):
    """Whatever idx_row_ptr and idx_pos hold: URCCO_OK, the run ends, no access leaves the arrays (HIPSIM_GUARD).  Values: 0 <= KE <= K <= n_events.
    Entries outside the stream take no part in the ranking: with distinct positions otherwise, the restatement still holds."""
    rng = np.random.default_rng(67)
    counts = [4200, 40, 700, 65, 64, 63, 1, 0, 2000, 100, 20, 7]
    n, n_users = sum(counts), len(counts)
    users = np.repeat(np.arange(n_users, dtype=np.int32), counts)[rng.permutation(n)]
    rp, pos = T.host_index(users, n_users, rng)
    items = rng.integers(0, 50, n).astype(np.int32)
    times = (T0 + rng.integers(-20, 20, n)).astype(np.int64)
    bad_pos = pos.copy()
    bad_pos[rng.permutation(n)[:500]] = np.array([-1, n, I32_MAX, -(1 << 31)], np.int32)[rng.integers(0, 4, 500)]
    bad_pos[[0, 63, 64, n - 1]] = (-1, n, I32_MAX, n)
    descending = rp[::-1].copy()
    beyond = rp + np.arange(n_users + 1) * 2400                       # row starts beyond the entries
    jumpy = rp.copy()
    jumpy[[2, 5, 7]] = (-50, 1 << 40, I64_MIN)
    drop = np.array([0, 3, 3, n_users - 1, 5], np.int32)
    for cap in (1, 30, 64, 1000):
        for name, h_rp, h_pos in (("pos", rp, bad_pos), ("descending", descending, pos), ("beyond", beyond, pos), ("jumpy", jumpy, bad_pos), ("both", beyond[::-1].copy(), bad_pos)):
            for d in (drop, np.zeros(0, np.int32)):
                t = T.TrimProblem(f"hostile {name}", n_users, items, times, h_rp, h_pos, T0, d)
                status, _, _, _, _, counts = run_cap(sess, t, cap, (n, n))
                assert status == _lib.OK and 0 <= counts[1] <= counts[0] <= n, (name, counts)
        t = T.TrimProblem("hostile pos, exact", n_users, items, times, rp, bad_pos, I64_MIN, np.zeros(0, np.int32))
        w = np.count_nonzero(~capped_ref(n, times, n_users, rp, bad_pos, cap))
        status, _, _, _, _, counts = run_cap(sess, t, cap, (n, n))
        assert status == _lib.OK and counts[0] == w < n, (cap, counts, w)


# ---- bad arguments --------------------------------------------------------------------------------------------------------------------------------
def bad_argument_cases(sess):
    lib = sess.lib
    t = T.make_word_problem(129, True, "random")
    n, nu = t.n_events, t.n_users
    d = dict(items=put(sess, t.items), times=put(sess, t.times), rp=put(sess, t.row_ptr), pos=put(sess, t.pos), drop=put(sess, t.drop),
             o_items=sess.empty(n, torch.int32), o_times=sess.empty(n, torch.int64), o_rp=sess.empty(nu + 1, torch.int64), o_pos=sess.empty(n, torch.int32),
             counts=sess.empty(2, torch.int64))
    ok = dict(s=sess.handle, n=n, nu=nu, min_time=t.min_time, n_drop=t.drop.size, cap=5, **{k: v.data_ptr() for k, v in d.items()})

    def call(**kw):
        a = dict(ok, **kw)
        return lib.urcco_dev_history_cap(a["s"], a["n"], a["items"], a["times"], a["nu"], a["rp"], a["pos"], a["min_time"], a["n_drop"], a["drop"], a["cap"], a["o_items"],
                                         a["o_times"], a["o_rp"], a["o_pos"], a["counts"])

    assert call() == _lib.OK
    for cap in (0, -1, -(1 << 31)):                                                  # max_per_user < 1
        assert call(cap=cap) == _lib.BAD_ARG, cap
    assert call(cap=1) == _lib.OK and call(cap=I32_MAX) == _lib.OK
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
    assert call(nu=0, rp=None, n_drop=0, drop=None) == _lib.OK
    sess.synchronize()
    assert int(d["o_rp"][0]) == 0 and int(d["counts"][1]) == 0 and int(d["counts"][0]) == np.count_nonzero(t.times >= t.min_time)
    assert call(n=0, items=None, pos=None, o_items=None, o_pos=None) == _lib.OK
    assert call(n=0, items=None, times=None, nu=0, rp=None, pos=None, n_drop=0, drop=None, o_items=None, o_times=None, o_pos=None) == _lib.OK
    sess.synchronize()
    assert int(d["o_rp"][0]) == 0 and d["counts"].tolist() == [0, 0]
    assert lib.urcco_version() == 305


# ---- the Python level -----------------------------------------------------------------------------------------------------------------------------
def host_cap(users, times, n_users, cap):
    """bool [n]: the events of a stream the cap keeps, from the users array"""
    n = users.size
    inside = np.flatnonzero((users >= 0) & (users < n_users))
    order = inside[np.argsort(users[inside], kind="stable")].astype(np.int32)
    return ~capped_ref(n, times, n_users, row_ptr_ref(users, n_users), order, cap)


def _dev(sess, streams):
    return {ev: tuple(put(sess, a) if a is not None else None for a in x) for ev, x in streams.items()}


def rows_unchanged_case(sess):
    """history_rows term rows of every user with max_items <= cap: bit-identical before and after trim(max_events_per_user=cap)"""
    from universal_recommender_amd.history import DeviceHistory
    algo, model = H.predict_stack(sess, 3000, 400, 250)
    n_users = 200
    streams, _ = H.make_stream_history(43, n_users, 400, 250)
    cap = 8
    cnt = np.bincount(streams["purchase"][0][streams["purchase"][0] >= 0], minlength=n_users)
    assert (cnt > cap).any() and (cnt <= cap).any()
    dh = DeviceHistory.from_streams(sess, model, _dev(sess, streams), n_users=n_users)
    q = put(sess, np.arange(n_users, dtype=np.int32))

    def term_rows(max_items):
        events = [(st.n_cols, max_items, False, st.idx_row_ptr, st.idx_pos, st.items, st.times, st.col_map) for st in dh.types.values()]
        terms, _, _ = sess.history_rows(q, n_users, events, 400, None)
        sess.synchronize()
        return [(rp.cpu().numpy(), ci.cpu().numpy()[: int(rp[-1])]) for rp, ci in terms]

    before = {m: term_rows(m) for m in (1, 3, cap)}
    assert dh.trim(max_events_per_user=cap) is dh
    assert all(after <= min(b, n_users * cap) for b, after in dh.last_trim.values()) and any(after < b for b, after in dh.last_trim.values())
    for m, want in before.items():
        got = term_rows(m)
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got, want)), m


def predict_case(sess):
    """DeviceHistory.trim(max_events_per_user=...) against from_streams over the host-filtered streams: term and exclusion rows through batch_predict
    and user_recommendations.  An int caps every type; a dict the types it names; the cap together with the other two rules."""
    from universal_recommender_amd.history import DeviceHistory
    algo, model = H.predict_stack(sess, 3000, 400, 250)
    n_users = 200
    streams, _ = H.make_stream_history(43, n_users, 400, 250)
    t = streams["purchase"][2]
    cut, drop = int(np.sort(t)[t.size // 4]), [0, 5, 77]
    qs = [{"user": u} for u in range(0, n_users, 3)] + [{"user": u, "item": int(u * 2)} for u in range(1, n_users, 7)] + [{"user": u, "userBias": -1.0, "num": 5} for u in range(2, 60, 5)]
    qs += [{"user": 999}, {}, {"item": 5}] + [{"user": u} for u in drop]
    for arg, cut_, drop_ in ((6, None, None), ({"purchase": 4}, None, None), ({ev: 5 + k for k, ev in enumerate(streams)}, cut, drop)):
        caps = arg if isinstance(arg, dict) else {ev: arg for ev in streams}
        want = {}
        for ev, (u, i, tm) in streams.items():
            keep = np.ones(u.size, bool)
            if ev in caps:
                keep &= host_cap(u, tm, n_users, caps[ev])
            if drop_ is not None:
                keep &= ~np.isin(u, drop_)
            if cut_ is not None and tm is not None:
                keep &= tm >= cut_
            want[ev] = (u[keep], i[keep], tm[keep] if tm is not None else None)
        dh = DeviceHistory.from_streams(sess, model, _dev(sess, streams), n_users=n_users).trim(before_ms=cut_, drop_users=drop_, max_events_per_user=arg)
        whole = DeviceHistory.from_streams(sess, model, _dev(sess, want), n_users=n_users)
        touched = [ev for ev in streams if ev in caps or drop_ is not None or (cut_ is not None and streams[ev][2] is not None)]
        assert dh.last_trim == {ev: (streams[ev][0].size, want[ev][0].size) for ev in touched}, (arg, dh.last_trim)
        assert any(want[ev][0].size < streams[ev][0].size for ev in caps)
        for ev in streams:
            n = want[ev][0].size
            assert dh.types[ev].n_events == n and np.array_equal(dh.types[ev].items.cpu().numpy()[:n], want[ev][1]), ev
        for weights in (None, "idf"):
            for blacklist in (None, ["purchase", "view"]):
                algo.ap.blacklistEvents = blacklist
                try:
                    res = algo.batch_predict(model, qs, whole, term_weights=weights)
                    assert algo.batch_predict(model, qs, dh, term_weights=weights) == res
                finally:
                    algo.ap.blacklistEvents = None
        assert any(s["score"] > 0 for r in res for s in r["itemScores"])
        assert all(torch.equal(a, b) for a, b in zip(algo.user_recommendations(model, dh), algo.user_recommendations(model, whole)))
    dh = DeviceHistory.from_streams(sess, model, _dev(sess, streams), n_users=n_users)
    for bad in (0, -3, 1 << 31, {"no such event": 3}, {"purchase": 0}):
        try:
            dh.trim(max_events_per_user=bad)
        except ValueError:
            continue
        raise AssertionError(f"trim(max_events_per_user={bad!r}) did not raise")
    assert all(dh.types[ev].n_events == streams[ev][0].size for ev in streams)      # nothing was modified


class CappedHost(L.HostHistory):
    """history_lifecycle_cases' host model with the cap rule"""

    def cap(self, caps):
        for ev, c in caps.items():
            u, i, t = self.streams[ev]
            keep = host_cap(u, t, self.n_users, c)
            self.streams[ev] = (u[keep], i[keep], t[keep] if t is not None else None)


def schedule_case(sess):
    """append, cap, append, trim(time), cap on ONE DeviceHistory, after every step against the host model: the state (streams and indexes), the history
    rows at caps below, at and above the counts, and batch_predict against the dict form"""
    from universal_recommender_amd.history import DeviceHistory
    rng = np.random.default_rng(101)
    stack = L.stack_for(sess)
    algo, model = stack
    planted = [L.SR_LDS + 4, 300, 65, 64, 63, 1, 0]
    n0 = len(planted) + 300
    counts = planted + rng.integers(0, 30, 300).tolist()
    early, late = (0, 200), (100, 300)
    some = lambda n: rng.integers(len(planted), n0, n)      # noqa: E731
    steps = [("create", {"purchase": L._events(rng, np.repeat(np.arange(n0), counts), L.N_ITEMS, early, negative=4), "view": L._events(rng, some(1500), L.N_VIEW, early)}),
             ("append", {"purchase": L._events(rng, some(2000), L.N_ITEMS, early), "wish": L._events(rng, np.concatenate([some(500), np.full(200, 1)]), L.N_ITEMS)}),
             ("cap", 64),
             ("append", {"purchase": L._events(rng, np.concatenate([some(1500), np.full(100, 0), np.full(70, 2)]), L.N_ITEMS, late), "view": L._events(rng, some(700), L.N_VIEW, late),
                         "wish": L._events(rng, np.concatenate([some(300), np.full(150, 1)]), L.N_ITEMS)}),
             ("time", L.T0 + L.TICK * 100),
             ("cap", {"purchase": 20, "wish": 100})]
    h = CappedHost()
    sched = L.Schedule(False, [], list(range(len(planted))), n0)
    q_users = L.query_users(sched)
    col_map = L.view_col_map()
    dh = None
    for op, arg in steps:
        before = {ev: h.n_events(ev) for ev in h.streams}
        if op in ("create", "append"):
            batch = L._device_batch(sess, arg, False)
            if dh is None:
                dh = DeviceHistory.from_streams(sess, model, batch, n_users=n0)
            else:
                assert dh.append(batch, n_users=n0) is dh
            h.append(arg, n0)
        elif op == "cap":
            caps = arg if isinstance(arg, dict) else {ev: arg for ev in h.streams}
            assert dh.trim(max_events_per_user=arg) is dh
            h.cap(caps)
            assert dh.last_trim == {ev: (before[ev], h.n_events(ev)) for ev in caps}, dh.last_trim
            assert any(h.n_events(ev) < before[ev] for ev in caps) and all(h.counts(ev).max() <= c for ev, c in caps.items())
        else:
            assert dh.trim(before_ms=arg) is dh
            h.trim(arg)
            assert all(0 < h.n_events(ev) < before[ev] for ev in ("purchase", "view"))
        if "view" in dh.types and dh.types["view"].col_map is None:
            dh.types["view"].col_map = put(sess, col_map)
        sess.synchronize()
        L.check_state(dh, h)
        L.check_rows(sess, dh, h, q_users, col_map)
        L.check_predict(stack, dh, h, sched)
    assert h.counts("purchase").max() == 20 and h.counts("wish").max() == 100


# ---- the larger shape (GPU) -----------------------------------------------------------------------------------------------------------------------
def larger_shape_case(sess):
    """2^20 + 77 events over 2^16 users, Zipf(1.3), cap 64: users of every class, the heaviest beyond 4096 events"""
    rng = np.random.default_rng(37)
    n, n_users, cap = (1 << 20) + 77, 1 << 16, 64
    users = ((rng.zipf(1.3, n) - 1) % n_users).astype(np.int32)
    users[rng.integers(0, n, 500)] = -1
    cnt = np.bincount(users[users >= 0], minlength=n_users)
    assert cnt.max() > 4096 and (cnt <= cap).any() and ((cnt > cap) & (cnt <= 4096)).any() and (cnt > 4096).any()      # nothing to do, one block in LDS, keys in global memory
    times = (T0 + rng.integers(-1000, 1000, n)).astype(np.int64)
    rp, pos = T.host_index(users, n_users, rng)
    t = T.TrimProblem("larger shape", n_users, rng.integers(-1, 1 << 20, n).astype(np.int32), times, rp, pos, T0 - 500, np.array([3, 70000, -1], np.int32))
    _, k, ke = check_cap(sess, t, cap)
    assert 0 < ke < k < n // 2
    t.min_time, t.drop = I64_MIN, np.zeros(0, np.int32)
    _, k, ke = check_cap(sess, t, cap)
    assert ke == np.minimum(cnt, cap).sum() and k == ke + np.count_nonzero(users < 0)
