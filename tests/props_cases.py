"""urcco_dev_props_* (decision D25 of DESIGN.md, include/urcco.h): the problems and checks that tests/test_sim_props.py and tests/test_gpu_props.py share.
The reference is tests/props_ref.py, the rule restated in plain Python over the list of events.  Every comparison is exact: the state words, row_ptr,
col_idx, the dates and the mask.

Every array goes to the device in a tensor of exactly its size and every output is allocated at exactly its size plus `pad` sentinel entries: a read or
write past either end faults under HIPSIM_GUARD, and the checks assert that the padding still holds the sentinel."""
import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

import props_ref as P
from history_append_cases import put
from universal_recommender_amd import _lib, ingest

I64_MIN, I64_MAX = P.I64_MIN, P.I64_MAX
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
SET, UNSET = _lib.PROP_SET, _lib.PROP_UNSET
SENTINEL = -77
T0 = 1_600_000_000_000
CLASS_EDGES = (0, 1, 63, 64, 65, 4096, 4097, 8193)     # lengths of a winner's list around the classes of the sorted-rows unit (csrc/cco_sorted_rows.h)


@dataclass
class Prop:
    """One property's stream.  lists[p] = the value ids of position p (a list property) or dates[p] = its date (a date property)."""
    items: np.ndarray                        # int32 [n]
    times: np.ndarray                        # int64 [n]
    kinds: Optional[np.ndarray]              # uint8 [n] or None: all SET
    lists: Optional[List[List[int]]] = None
    dates: Optional[np.ndarray] = None
    n_cols: int = 0

    @property
    def n(self):
        return int(self.items.size)

    def kinds_or_set(self):
        return self.kinds if self.kinds is not None else np.zeros(self.n, np.uint8)

    def events(self):
        return list(zip(self.items.tolist(), self.times.tolist(), self.kinds_or_set().tolist()))


@dataclass
class Store:
    n_items: int
    props: Dict[str, Prop]
    del_items: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    del_times: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))


def prop(events, lists=None, dates=None, n_cols=0, all_set=False):
    """events: (item, time, kind) tuples"""
    items = np.array([e[0] for e in events], np.int32)
    times = np.array([e[1] for e in events], np.int64)
    kinds = None if all_set else np.array([e[2] for e in events], np.uint8)
    return Prop(items, times, kinds, lists, None if dates is None else np.asarray(dates, np.int64), n_cols)


# ---- the calls, through ctypes ------------------------------------------------------------------------------------------------------------------------
def zeros(sess, n, dtype):
    t = sess.empty(n, dtype)
    if n:
        t.zero_()
    return t


class DevState:
    """The state arrays of one property at exactly n_items entries, all-zero"""

    def __init__(self, sess, n_items):
        self.sess, self.n_items = sess, n_items
        self.t_set, self.pos_set, self.t_unset = zeros(sess, n_items, torch.int64), zeros(sess, n_items, torch.int32), zeros(sess, n_items, torch.int64)
        self.n_events = 0

    def apply(self, p: Prop, lo: int, hi: int):
        s = self.sess
        items, times = put(s, p.items[lo:hi]), put(s, p.times[lo:hi])
        kinds = None if p.kinds is None else put(s, p.kinds[lo:hi])
        st = s.lib.urcco_dev_props_apply(s.handle, self.n_items, hi - lo, items.data_ptr() if hi > lo else None, times.data_ptr() if hi > lo else None,
                                         kinds.data_ptr() if kinds is not None and hi > lo else None, lo, self.t_set.data_ptr() if self.n_items else None,
                                         self.pos_set.data_ptr() if self.n_items else None, self.t_unset.data_ptr() if self.n_items else None)
        s.synchronize()
        assert st == _lib.OK, (st, lo, hi)
        self.n_events = max(self.n_events, hi)

    def grown(self, n_items):
        """the zero-extended state of a catalogue that grew"""
        out = DevState(self.sess, n_items)
        out.n_events = self.n_events
        for a in ("t_set", "pos_set", "t_unset"):
            getattr(out, a)[: self.n_items].copy_(getattr(self, a))
        return out

    def words(self):
        return (self.t_set.cpu().numpy().view(np.uint64).copy(), self.pos_set.cpu().numpy().view(np.uint32).copy(), self.t_unset.cpu().numpy().view(np.uint64).copy())

    def struct(self, t_del):
        n = self.n_items
        return _lib.PropState(self.t_set.data_ptr() if n else None, self.pos_set.data_ptr() if n else None, self.t_unset.data_ptr() if n else None,
                              t_del.data_ptr() if t_del is not None and n else None, self.n_events)


def run_delete(sess, n_items, items, times, t_del=None):
    t_del = zeros(sess, n_items, torch.int64) if t_del is None else t_del
    n = int(items.size)
    d_i, d_t = put(sess, items), put(sess, times)
    st = sess.lib.urcco_dev_props_delete(sess.handle, n_items, n, d_i.data_ptr() if n else None, d_t.data_ptr() if n else None, t_del.data_ptr() if n_items else None)
    sess.synchronize()
    assert st == _lib.OK
    return t_del


def value_arrays(p: Prop):
    vp = np.zeros(p.n + 1, np.int64)
    np.cumsum([len(v) for v in p.lists], out=vp[1:])
    return vp, np.array([v for vs in p.lists for v in vs], np.int32)


def run_rows(sess, st: DevState, t_del, p: Prop, capacity=None, pad=0):
    """urcco_dev_props_bounds, then urcco_dev_props_rows with capacity(bound row_ptr) entries (None: the bound total).  Returns (bound row_ptr, capacity,
    final row_ptr, col_idx with its padding)"""
    n = st.n_items
    vp, vals = value_arrays(p)
    vp, vals = vp[: st.n_events + 1], vals[: vp[st.n_events]]
    d_vp, d_vals = put(sess, vp), put(sess, vals)
    state = st.struct(t_del)
    rp = sess.empty(n + 1, torch.int64)
    rp.fill_(SENTINEL)
    status = sess.lib.urcco_dev_props_bounds(sess.handle, n, C.byref(state), d_vp.data_ptr(), int(vals.size), rp.data_ptr())
    sess.synchronize()
    assert status == _lib.OK
    bound_rp = rp.cpu().numpy().copy()
    cap = int(bound_rp[n]) if capacity is None else int(capacity(bound_rp))
    ci = sess.empty(max(cap, 1) + pad, torch.int32)
    ci.fill_(SENTINEL)
    status = sess.lib.urcco_dev_props_rows(sess.handle, n, C.byref(state), d_vp.data_ptr(), d_vals.data_ptr() if vals.size else None, int(vals.size), p.n_cols,
                                           rp.data_ptr(), ci.data_ptr(), cap)
    sess.synchronize()
    assert status == _lib.OK
    return bound_rp, cap, rp.cpu().numpy(), ci.cpu().numpy()


def run_dates(sess, st: DevState, t_del, p: Prop, pad=0):
    n = st.n_items
    d_v = put(sess, p.dates[: st.n_events])
    out = sess.empty(max(n, 1) + pad, torch.int64)
    out.fill_(SENTINEL)
    state = st.struct(t_del)
    status = sess.lib.urcco_dev_props_dates(sess.handle, n, C.byref(state), d_v.data_ptr() if st.n_events else None, out.data_ptr())
    sess.synchronize()
    assert status == _lib.OK
    return out.cpu().numpy()


def run_exists(sess, n_items, t_del, t_sets, pad=0):
    out = sess.empty(max(n_items, 1) + pad, torch.uint8)
    out.fill_(7)
    ptrs = (C.c_void_p * max(len(t_sets), 1))(*[t.data_ptr() for t in t_sets])
    status = sess.lib.urcco_dev_props_exists(sess.handle, n_items, t_del.data_ptr() if n_items else None, ptrs, len(t_sets), out.data_ptr())
    sess.synchronize()
    assert status == _lib.OK
    return out.cpu().numpy()


def csr_pairs(sess, pr, pc, n_rows, n_cols):
    """urcco_dev_csr_from_pairs over the pairs: (row_ptr, col_idx[:nnz])"""
    if pr.size == 0:
        return np.zeros(n_rows + 1, np.int64), np.zeros(0, np.int32)
    m = ingest.csr_from_pairs(sess, put(sess, pr), put(sess, pc), n_rows, n_cols)
    return m.row_ptr.cpu().numpy(), m.col_idx[: m.nnz_bound].cpu().numpy()


# ---- the checks -------------------------------------------------------------------------------------------------------------------------------------
def batches(n, k):
    """cut points of k batches over n events, the first and every third one empty when k > 2"""
    if k == 1:
        return [0, n]
    cuts = sorted(int(round(j * n / k)) for j in range(k + 1))
    if k > 2:
        cuts[1] = 0
        for j in range(3, k, 3):
            cuts[j] = cuts[j - 1]
    return cuts


def apply_in(sess, n_items, p: Prop, cuts):
    st = DevState(sess, n_items)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        st.apply(p, lo, hi)
    return st


def check_store(sess, name, s: Store, ks=(1, 2, 7), pad=3, pairs=True):
    """Every property of the store applied in 1, 2 and 7 batches: the state words equal the reference's bit for bit; from the state the rows (equal to the
    reference's and to urcco_dev_csr_from_pairs over the alive winners' pairs), the dates and the mask.  Returns the reference's (S, U) per property, D, and
    the results of the last batching."""
    n = s.n_items
    D = P.aggregate_deletes(n, zip(s.del_items.tolist(), s.del_times.tolist()))
    t_del = run_delete(sess, n, s.del_items, s.del_times)
    assert np.array_equal(t_del.cpu().numpy().view(np.uint64), P.delete_words(n, D)), name
    refs, out, t_sets = {}, {}, []
    for pname, p in s.props.items():
        S, U = P.aggregate(n, p.events())
        refs[pname] = (S, U)
        want = P.state_words(n, S, U)
        win = P.winners(n, S, U, D)
        for k in ks:
            st = apply_in(sess, n, p, batches(p.n, k))
            got = st.words()
            for a, b, what in zip(got, want, ("t_set", "pos_set", "t_unset")):
                assert np.array_equal(a, b), (name, pname, k, what, a[:8], b[:8])
            if p.lists is not None:
                w_rp, w_ci, (pr, pc) = P.rows_of(n, win, p.lists, p.n_cols)
                _, cap, rp, ci = run_rows(sess, st, t_del, p, pad=pad)
                assert np.array_equal(rp, w_rp), (name, pname, k, rp[:10], w_rp[:10])
                assert np.array_equal(ci[: w_rp[n]], w_ci), (name, pname, k)
                assert (ci[max(cap, 1):] == SENTINEL).all(), f"{name}: written at or past col_idx[capacity]"
                if pairs and k == ks[0]:
                    c_rp, c_ci = csr_pairs(sess, pr, pc, n, max(p.n_cols, 1))
                    assert np.array_equal(rp, c_rp) and np.array_equal(ci[: w_rp[n]], c_ci), (name, pname, "csr_from_pairs")
                out[pname] = (rp, ci[: w_rp[n]])
            else:
                got_d = run_dates(sess, st, t_del, p, pad=pad)
                assert np.array_equal(got_d[:n], P.dates_of(n, win, p.dates)), (name, pname, k)
                assert (got_d[max(n, 1):] == SENTINEL).all(), f"{name}: written at or past out[n_items]"
                out[pname] = got_d[:n]
        t_sets.append(st.t_set)
    mask = run_exists(sess, n, t_del, t_sets, pad=pad)
    w_mask = P.exists_mask(n, [S for S, _ in refs.values()], D)
    assert np.array_equal(mask[:n], w_mask), (name, mask[:16], w_mask[:16])
    assert (mask[max(n, 1):] == 7).all(), f"{name}: written at or past out_mask[n_items]"
    return refs, D, out, mask[:n]


def random_prop(rng, n_items, n, n_cols, t_lo=T0, t_hi=T0 + 50, unset=0.3, max_len=4, date=False, distinct_times=False, stray=True):
    items = rng.integers(0, n_items, n).astype(np.int32) if n_items else np.zeros(n, np.int32)
    if stray and n:
        at = rng.integers(0, n, max(n // 20, 1))
        items[at] = np.array([-1, n_items, I32_MIN, I32_MAX], np.int32)[rng.integers(0, 4, at.size)]
    times = (t_lo + rng.permutation(n)).astype(np.int64) if distinct_times else rng.integers(t_lo, t_hi, n).astype(np.int64)
    kinds = (rng.random(n) < unset).astype(np.uint8)
    if date:
        return Prop(items, times, kinds, None, rng.integers(-5, 10**12, n).astype(np.int64), 0)
    lists = [[] if k == UNSET else rng.integers(-1, n_cols + 2, rng.integers(0, max_len + 1)).tolist() for k in kinds]
    return Prop(items, times, kinds, lists, None, n_cols)


def tie_cases(sess):
    """The ties and the revival the rule names, each with the outcome written out"""
    t = T0
    # item 0: set and unset at one millisecond -> dead.  item 1: set and delete at one millisecond -> dead and deleted.  item 2: two sets at one millisecond ->
    # the later position wins.  item 3: delete, then a later set of "cat" only -> cat alive, "tag" dead, not deleted.  item 4: an unset of a key never set.
    # item 5: set later than its unset -> alive.  item 6: only a delete -> deleted.  item 7: nothing at all.
    cat = prop([(0, t, SET), (0, t, UNSET), (1, t, SET), (2, t, SET), (2, t, SET), (3, t - 5, SET), (3, t + 9, SET), (4, t, UNSET), (5, t, UNSET), (5, t + 1, SET)],
               lists=[[1], [], [2], [3], [4, 0], [5], [6, 6, 1], [], [], [2, 0]], n_cols=7)
    tag = prop([(3, t - 5, SET), (1, t - 1, SET), (2, t + 3, SET)], lists=[[0], [1], [2]], n_cols=3)
    day = prop([(3, t - 5, SET), (2, t, SET), (2, t, SET), (5, t, SET), (5, t, UNSET)], dates=[11, 22, 33, 44, 55])
    s = Store(8, {"cat": cat, "tag": tag, "day": day}, np.array([1, 3, 6], np.int32), np.array([t, t, t - 100], np.int64))
    refs, D, out, mask = check_store(sess, "ties", s)
    rp, ci = out["cat"]
    rows = [ci[rp[i]:rp[i + 1]].tolist() for i in range(8)]
    assert rows == [[], [], [0, 4], [1, 6], [], [0, 2], [], []], rows
    rp, ci = out["tag"]
    assert [ci[rp[i]:rp[i + 1]].tolist() for i in range(8)] == [[], [], [2], [], [], [], [], []]
    assert out["day"].tolist() == [I64_MIN, I64_MIN, 33, I64_MIN, I64_MIN, I64_MIN, I64_MIN, I64_MIN]
    assert mask.tolist() == [1, 0, 1, 1, 1, 1, 0, 1]
    # two sets at one millisecond across two batches: the later position wins whichever batch it is in
    two = prop([(0, t, SET), (1, t + 1, SET), (0, t, SET), (1, t, SET)], lists=[[1], [2], [3], [4]], n_cols=5)
    st = DevState(sess, 2)
    st.apply(two, 0, 2)
    st.apply(two, 2, 4)
    assert st.words()[1].tolist() == [3, 2]
    _, _, rp, ci = run_rows(sess, st, None, two)
    assert rp.tolist() == [0, 1, 2] and ci[:2].tolist() == [3, 2]


def batching_cases(sess):
    rng = np.random.default_rng(5)
    for n_items, n in ((1, 40), (50, 700), (300, 2500)):
        s = Store(n_items, {"a": random_prop(rng, n_items, n, 9), "b": random_prop(rng, n_items, n // 2 + 1, 300, max_len=80, unset=0.1),
                            "d": random_prop(rng, n_items, n, 0, date=True)},
                  rng.integers(-1, n_items + 1, n_items // 3 + 1).astype(np.int32), rng.integers(T0, T0 + 50, n_items // 3 + 1).astype(np.int64))
        check_store(sess, f"batching {n_items}", s)
    # pairwise distinct times: any permutation of the stream gives the same rows and dates
    n_items, n = 40, 600
    a, d = random_prop(rng, n_items, n, 12, distinct_times=True), random_prop(rng, n_items, n, 0, date=True, distinct_times=True)
    s = Store(n_items, {"a": a, "d": d}, np.array([3, 5], np.int32), np.array([T0 + 100, T0 + 300], np.int64))
    _, _, base, _ = check_store(sess, "permutation base", s, ks=(1,))
    for _ in range(3):
        perm = rng.permutation(n)
        pa = Prop(a.items[perm], a.times[perm], a.kinds[perm], [a.lists[j] for j in perm], None, a.n_cols)
        pd = Prop(d.items[perm], d.times[perm], d.kinds[perm], None, d.dates[perm], 0)
        _, _, out, _ = check_store(sess, "permutation", Store(n_items, {"a": pa, "d": pd}, s.del_items, s.del_times), ks=(1, 7))
        assert np.array_equal(out["a"][0], base["a"][0]) and np.array_equal(out["a"][1], base["a"][1]) and np.array_equal(out["d"], base["d"])


def domain_cases(sess):
    rng = np.random.default_rng(6)
    edge_t = [I64_MIN, I64_MIN + 1, -1, 0, I64_MAX]
    for n_items in (0, 1, 63, 64, 65):
        ids = [-1, n_items, I32_MIN, I32_MAX] + list(range(min(n_items, 3))) + ([n_items - 1] if n_items else [])
        ev = [(i, t, k) for i in ids for t in edge_t for k in (SET, UNSET)]
        ev = [ev[j] for j in rng.permutation(len(ev))]
        lists = [[j % 5] for j in range(len(ev))]
        a = prop(ev, lists=lists, n_cols=5)
        d = prop(ev, dates=rng.integers(-9, 9, len(ev)))
        dl = [(i, t) for i in ids for t in edge_t[:3]]
        s = Store(n_items, {"a": a, "d": d}, np.array([x[0] for x in dl], np.int32), np.array([x[1] for x in dl], np.int64))
        refs, D, _, _ = check_store(sess, f"domain {n_items}", s)
        assert all(t != I64_MIN for S, U in refs.values() for t, _ in S.values()) and I64_MIN not in D.values()     # INT64_MIN is ignored, not a time
    # every edge time on its own: INT64_MIN leaves the state zero, the others order as signed numbers
    for k, t in enumerate(edge_t):
        st = apply_in(sess, 2, prop([(0, t, SET), (1, t, UNSET)], lists=[[0], []], n_cols=1), [0, 2])
        assert st.words()[0].tolist() == [t + (1 << 63) if k else 0, 0] and st.words()[2].tolist() == [0, t + (1 << 63) if k else 0]
    asc = prop([(0, t, SET) for t in edge_t[1:]], lists=[[j] for j in range(4)], n_cols=4)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        p = Prop(asc.items[order], asc.times[order], None, [asc.lists[j] for j in order], None, 4)
        st = apply_in(sess, 1, p, [0, 4])
        _, _, rp, ci = run_rows(sess, st, None, p)
        assert ci[: rp[1]].tolist() == [3], order              # INT64_MAX is the latest
    # the catalogue grows between two batches: the zero-extended state is the state of the whole stream over the larger catalogue
    n0, n1, n = 40, 70, 400
    p = random_prop(rng, n1, n, 6)
    first = p.items[: n // 2]
    first[(first >= n0) & (first < n1)] -= n0 - 5                # the first half names items of the small catalogue (or none at all)
    st = apply_in(sess, n0, p, [0, n // 2]).grown(n1)
    st.apply(p, n // 2, n)
    want = P.state_words(n1, *P.aggregate(n1, p.events()))
    for a, b in zip(st.words(), want):
        assert np.array_equal(a, b)
    t_del = run_delete(sess, n0, np.array([1, 2], np.int32), np.array([T0, T0 + 20], np.int64))
    big = zeros(sess, n1, torch.int64)
    big[:n0].copy_(t_del)
    big = run_delete(sess, n1, np.array([2, 60], np.int32), np.array([T0 + 10, T0], np.int64), big)
    assert np.array_equal(big.cpu().numpy().view(np.uint64), P.delete_words(n1, {1: T0, 2: T0 + 20, 60: T0}))


def edge_lists(rng, n_cols):
    """winner lists of the class-edge lengths, then the special rows: duplicates only, all equal, ids out of range only, alive but empty"""
    out = [rng.integers(0, n_cols, m).tolist() for m in CLASS_EDGES]
    out += [[5, 5, 7, 7, 5], [9] * 70, [-1, n_cols, I32_MAX, I32_MIN] * 20, [], [n_cols - 1, 0, -3, n_cols, 0] * 900]
    return out


def rows_cases(sess, n_cols=3000):
    rng = np.random.default_rng(7)
    lists = edge_lists(rng, n_cols)
    n_items = len(lists) + 3                                  # the last three: never set, unset later, superseded by a short list
    ev = [(i, T0 + i, SET) for i in range(len(lists))] + [(n_items - 2, T0, SET), (n_items - 2, T0 + 1, UNSET), (n_items - 1, T0, SET), (n_items - 1, T0 + 1, SET)]
    all_lists = lists + [rng.integers(0, n_cols, 100).tolist(), [], rng.integers(0, n_cols, 5000).tolist(), [4, 2]]
    order = rng.permutation(len(ev))
    p = prop([ev[j] for j in order], lists=[all_lists[j] for j in order], n_cols=n_cols)
    s = Store(n_items, {"rows": p})
    _, _, out, _ = check_store(sess, "rows", s, ks=(1, 2))
    rp, ci = out["rows"]
    assert (np.diff(rp)[: len(CLASS_EDGES)] <= np.array(CLASS_EDGES)).all() and rp[n_items] - rp[n_items - 1] == 2
    # the capacity contract: a row is written iff its bound ends within the capacity; nothing is written past it
    st = apply_in(sess, n_items, p, [0, p.n])
    full_rp, full_ci = rp, ci
    total = None
    for what in ("zero", "one short", "exact", "half"):
        capacity = {"zero": lambda b: 0, "one short": lambda b: int(b[-1]) - 1, "exact": lambda b: int(b[-1]), "half": lambda b: int(b[-1]) // 2}[what]
        bound, cap, rp2, ci2 = run_rows(sess, st, None, p, capacity, pad=5)
        total = int(bound[-1])
        assert total == sum(len(l) for i, l in enumerate(lists)) + 2
        fits = bound[1:] <= cap
        want = [full_ci[full_rp[i]:full_rp[i + 1]] if fits[i] else np.zeros(0, np.int32) for i in range(n_items)]
        w_rp = np.zeros(n_items + 1, np.int64)
        np.cumsum([w.size for w in want], out=w_rp[1:])
        assert np.array_equal(rp2, w_rp), (what, rp2, w_rp)
        assert np.array_equal(ci2[: w_rp[-1]], np.concatenate(want) if w_rp[-1] else np.zeros(0, np.int32)), what
        assert (ci2[max(cap, 1):] == SENTINEL).all(), f"{what}: written at or past col_idx[capacity]"
        if what == "one short":
            assert not fits[-1] and fits[: n_items - 1].any()


def malformed_state_cases(sess):
    """pos_set beyond the stream and val_ptr entries outside the value array: wrong rows are allowed, an access outside the arrays is not (HIPSIM_GUARD)"""
    p = prop([(0, T0, SET), (1, T0, SET), (2, T0, SET)], lists=[[1, 2], [3], [0, 1, 2, 3]], n_cols=4)
    st = apply_in(sess, 3, p, [0, 3])
    st.pos_set.copy_(torch.tensor([9, 2, -1], dtype=torch.int32))
    _, _, rp, ci = run_rows(sess, st, None, p, pad=2)
    assert rp.tolist() == [0, 0, 1, 1] and ci[:1].tolist() == [3]
    assert run_dates(sess, st, None, prop(p.events(), dates=[5, 6, 7]))[:3].tolist() == [I64_MIN, 6, I64_MIN]
    st = apply_in(sess, 3, p, [0, 3])
    state = st.struct(None)
    for vp in ([0, -5, 3, 99], [0, 9, 2, 7], [5, 4, 3, 2], [I64_MIN, I64_MAX, I64_MIN, I64_MAX]):
        d_vp, d_vals = put(sess, np.array(vp, np.int64)), put(sess, np.arange(7, dtype=np.int32))
        rp = sess.empty(4, torch.int64)
        assert sess.lib.urcco_dev_props_bounds(sess.handle, 3, C.byref(state), d_vp.data_ptr(), 7, rp.data_ptr()) == _lib.OK
        sess.synchronize()
        cap = int(rp[3])
        assert 0 <= cap <= 21
        ci = sess.empty(max(cap, 1), torch.int32)
        assert sess.lib.urcco_dev_props_rows(sess.handle, 3, C.byref(state), d_vp.data_ptr(), d_vals.data_ptr(), 7, 4, rp.data_ptr(), ci.data_ptr(), cap) == _lib.OK
        sess.synchronize()
        assert 0 <= int(rp[3]) <= cap


def contention_case(sess, n_hot=100_000, n_rest=100):
    """one item owns n_hot of the n_hot + n_rest events, its times shuffled: the read-before-atomic path under the heaviest contention"""
    rng = np.random.default_rng(8)
    n, n_items = n_hot + n_rest, 50
    items = np.full(n, 17, np.int32)
    items[rng.choice(n, n_rest, replace=False)] = rng.integers(0, n_items, n_rest).astype(np.int32)
    times = (T0 + rng.permutation(n) // 3).astype(np.int64)          # shuffled, every time three times: the position decides among equal times
    kinds = (rng.random(n) < 0.4).astype(np.uint8)
    lists = [[] if k else [int(j % 11), int(j % 7)] for j, k in enumerate(kinds)]
    s = Store(n_items, {"hot": Prop(items, times, kinds, lists, None, 11)}, np.full(300, 17, np.int32), (T0 + rng.permutation(n)[:300] // 6).astype(np.int64))
    check_store(sess, "contention", s, ks=(1, 7))


def bad_argument_cases(sess):
    lib, h = sess.lib, sess.handle
    n = 4
    st = DevState(sess, n)
    items, times, kinds = put(sess, np.zeros(3, np.int32)), put(sess, np.zeros(3, np.int64)), put(sess, np.zeros(3, np.uint8))
    ts, ps, tu = st.t_set.data_ptr(), st.pos_set.data_ptr(), st.t_unset.data_ptr()
    ip, tp, kp = items.data_ptr(), times.data_ptr(), kinds.data_ptr()
    BAD = _lib.BAD_ARG
    assert lib.urcco_dev_props_apply(h, n, 3, ip, tp, kp, 0, ts, ps, tu) == _lib.OK
    assert lib.urcco_dev_props_apply(h, n, 3, ip, tp, None, 0, ts, ps, tu) == _lib.OK
    assert lib.urcco_dev_props_apply(h, n, 3, ip, tp, kp, (1 << 31) - 4, ts, ps, tu) == _lib.OK          # pos_base + n_new = 2^31 - 1
    assert lib.urcco_dev_props_apply(h, n, 0, None, None, None, (1 << 31) - 1, ts, ps, tu) == _lib.OK
    assert lib.urcco_dev_props_apply(h, 0, 0, None, None, None, 0, None, None, None) == _lib.OK
    for args in ((None, n, 3, ip, tp, kp, 0, ts, ps, tu), (h, -1, 3, ip, tp, kp, 0, ts, ps, tu), (h, n, -1, ip, tp, kp, 0, ts, ps, tu), (h, n, 3, ip, tp, kp, -1, ts, ps, tu),
                 (h, n, 3, ip, tp, kp, (1 << 31) - 3, ts, ps, tu), (h, n, 1 << 31, ip, tp, kp, 0, ts, ps, tu), (h, n, 3, None, tp, kp, 0, ts, ps, tu),
                 (h, n, 3, ip, None, kp, 0, ts, ps, tu), (h, n, 3, ip, tp, kp, 0, None, ps, tu), (h, n, 3, ip, tp, kp, 0, ts, None, tu), (h, n, 3, ip, tp, kp, 0, ts, ps, None),
                 (h, n, 0, None, None, None, 0, None, ps, tu)):
        assert lib.urcco_dev_props_apply(*args) == BAD, args
    td = zeros(sess, n, torch.int64)
    assert lib.urcco_dev_props_delete(h, n, 3, ip, tp, td.data_ptr()) == _lib.OK
    assert lib.urcco_dev_props_delete(h, 0, 0, None, None, None) == _lib.OK
    for args in ((None, n, 3, ip, tp, td.data_ptr()), (h, -1, 3, ip, tp, td.data_ptr()), (h, n, -1, ip, tp, td.data_ptr()), (h, n, 1 << 31, ip, tp, td.data_ptr()),
                 (h, n, 3, None, tp, td.data_ptr()), (h, n, 3, ip, None, td.data_ptr()), (h, n, 3, ip, tp, None)):
        assert lib.urcco_dev_props_delete(*args) == BAD, args
    st.n_events = 3
    vp, vals = put(sess, np.arange(4, dtype=np.int64)), put(sess, np.zeros(3, np.int32))
    rp, ci = sess.empty(n + 1, torch.int64), sess.empty(3, torch.int32)
    out, mask = sess.empty(n, torch.int64), sess.empty(n, torch.uint8)
    dv = put(sess, np.zeros(3, np.int64))

    def state(**kw):
        s = st.struct(td)
        for k, v in kw.items():
            setattr(s, k, v)
        return C.byref(s)
    good = state()
    assert lib.urcco_dev_props_bounds(h, n, good, vp.data_ptr(), 3, rp.data_ptr()) == _lib.OK
    assert lib.urcco_dev_props_bounds(h, n, state(t_del=None), vp.data_ptr(), 3, rp.data_ptr()) == _lib.OK
    assert lib.urcco_dev_props_bounds(h, n, state(n_events=0), None, 0, rp.data_ptr()) == _lib.OK
    bad_states = [None, state(t_set=None), state(pos_set=None), state(t_unset=None), state(n_events=-1), state(n_events=1 << 31)]
    for b in bad_states:
        assert lib.urcco_dev_props_bounds(h, n, b, vp.data_ptr(), 3, rp.data_ptr()) == BAD
        assert lib.urcco_dev_props_rows(h, n, b, vp.data_ptr(), vals.data_ptr(), 3, 5, rp.data_ptr(), ci.data_ptr(), 3) == BAD
        assert lib.urcco_dev_props_dates(h, n, b, dv.data_ptr(), out.data_ptr()) == BAD
    for args in ((None, n, good, vp.data_ptr(), 3, rp.data_ptr()), (h, -1, good, vp.data_ptr(), 3, rp.data_ptr()), (h, n, good, None, 3, rp.data_ptr()),
                 (h, n, good, vp.data_ptr(), -1, rp.data_ptr()), (h, n, good, vp.data_ptr(), 3, None)):
        assert lib.urcco_dev_props_bounds(*args) == BAD, args
    sess.synchronize()
    assert lib.urcco_dev_props_rows(h, n, good, vp.data_ptr(), vals.data_ptr(), 3, 5, rp.data_ptr(), ci.data_ptr(), 3) == _lib.OK
    for args in ((None, n, good, vp.data_ptr(), vals.data_ptr(), 3, 5, rp.data_ptr(), ci.data_ptr(), 3), (h, -1, good, vp.data_ptr(), vals.data_ptr(), 3, 5, rp.data_ptr(), ci.data_ptr(), 3),
                 (h, n, good, None, vals.data_ptr(), 3, 5, rp.data_ptr(), ci.data_ptr(), 3), (h, n, good, vp.data_ptr(), None, 3, 5, rp.data_ptr(), ci.data_ptr(), 3),
                 (h, n, good, vp.data_ptr(), vals.data_ptr(), -1, 5, rp.data_ptr(), ci.data_ptr(), 3), (h, n, good, vp.data_ptr(), vals.data_ptr(), 3, -1, rp.data_ptr(), ci.data_ptr(), 3),
                 (h, n, good, vp.data_ptr(), vals.data_ptr(), 3, 5, None, ci.data_ptr(), 3), (h, n, good, vp.data_ptr(), vals.data_ptr(), 3, 5, rp.data_ptr(), None, 3),
                 (h, n, good, vp.data_ptr(), vals.data_ptr(), 3, 5, rp.data_ptr(), ci.data_ptr(), -1)):
        assert lib.urcco_dev_props_rows(*args) == BAD, args
    assert lib.urcco_dev_props_dates(h, n, good, dv.data_ptr(), out.data_ptr()) == _lib.OK
    assert lib.urcco_dev_props_dates(h, n, state(n_events=0), None, out.data_ptr()) == _lib.OK
    for args in ((None, n, good, dv.data_ptr(), out.data_ptr()), (h, -1, good, dv.data_ptr(), out.data_ptr()), (h, n, good, None, out.data_ptr()), (h, n, good, dv.data_ptr(), None)):
        assert lib.urcco_dev_props_dates(*args) == BAD, args
    one = (C.c_void_p * 1)(ts)
    many = (C.c_void_p * 17)(*([ts] * 17))
    hole = (C.c_void_p * 2)(ts, None)
    assert lib.urcco_dev_props_exists(h, n, td.data_ptr(), one, 1, mask.data_ptr()) == _lib.OK
    assert lib.urcco_dev_props_exists(h, n, td.data_ptr(), None, 0, mask.data_ptr()) == _lib.OK
    assert lib.urcco_dev_props_exists(h, n, td.data_ptr(), many, 16, mask.data_ptr()) == _lib.OK
    assert lib.urcco_dev_props_exists(h, 0, None, None, 0, None) == _lib.OK
    for args in ((None, n, td.data_ptr(), one, 1, mask.data_ptr()), (h, -1, td.data_ptr(), one, 1, mask.data_ptr()), (h, n, None, one, 1, mask.data_ptr()),
                 (h, n, td.data_ptr(), None, 1, mask.data_ptr()), (h, n, td.data_ptr(), one, -1, mask.data_ptr()), (h, n, td.data_ptr(), many, 17, mask.data_ptr()),
                 (h, n, td.data_ptr(), hole, 2, mask.data_ptr()), (h, n, td.data_ptr(), one, 1, None)):
        assert lib.urcco_dev_props_exists(*args) == BAD, args
    sess.synchronize()


def numpy_reference_case():
    """tests/props_ref.py's numpy form against its plain-Python form: what the larger GPU shape is checked with"""
    rng = np.random.default_rng(9)
    for n_items, n in ((1, 30), (20, 500), (200, 3000)):
        p = random_prop(rng, n_items, n, 5, t_hi=T0 + 30)
        p.times[rng.integers(0, n, 5)] = I64_MIN
        S, U = P.aggregate(n_items, p.events())
        for a, b in zip(P.aggregate_np(n_items, p.items, p.times, p.kinds), P.state_words(n_items, S, U)):
            assert np.array_equal(a, b)
        di, dt = rng.integers(-1, n_items + 1, 40).astype(np.int32), rng.integers(T0, T0 + 30, 40).astype(np.int64)
        D = P.aggregate_deletes(n_items, zip(di.tolist(), dt.tolist()))
        t_del = P.delete_np(n_items, di, dt)
        assert np.array_equal(t_del, P.delete_words(n_items, D))
        t_set, pos_set, t_unset = P.aggregate_np(n_items, p.items, p.times, p.kinds)
        assert np.flatnonzero(P.alive_np(t_set, t_unset, t_del)).tolist() == sorted(P.winners(n_items, S, U, D))
        assert np.array_equal(P.exists_np([t_set], t_del), P.exists_mask(n_items, [S], D))
