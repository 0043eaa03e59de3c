"""urcco_dev_props_compact (decision D28 of DESIGN.md, include/urcco.h): the problems and checks that tests/test_sim_props_compact.py and
tests/test_gpu_props_compact.py share.  The contract, restated in numpy (compact_ref):

    win        = the distinct positions pos_set[i] - 1 inside 0 .. n_events, ascending;  K = their number;  new_of = the rank in win
    out_pos_set[i] = new_of[pos_set[i] - 1] + 1, 0 where pos_set[i] names no position;  out_old_pos = win
    lists:     len[j] = the clamped slice length of win[j] when the item naming it is alive, else 0;  out_val_ptr = min(scan(len), n_values);
               out_values = the slices' fronts in new order;  V = out_val_ptr[K]
    dates:     out_date_values = date_values[win];  counts = [K, V]

and the promise: every output of the store (`_bounds` / `_rows`, `_dates`, `_exists`) over the compacted stream equals, bit for bit, the one over the
stream as it was, and t_set / t_unset / t_del are untouched.  Every array goes to the device at exactly its size and every output is allocated at
exactly K / K + 1 / V entries plus `pad` sentinel entries: a read or write past either end faults under HIPSIM_GUARD."""
import ctypes as C

import numpy as np
import torch

import props_cases as PC
import props_ref as P
from history_append_cases import put
from universal_recommender_amd import _lib

I64_MIN, I64_MAX, I32_MAX = PC.I64_MIN, PC.I64_MAX, PC.I32_MAX
SET, UNSET = PC.SET, PC.UNSET
SENTINEL = PC.SENTINEL
T0 = PC.T0


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------
def compact_ref(n_items, words, t_del, n_events, vp=None, vals=None, dates=None):
    """words: (t_set uint64, pos_set uint32, t_unset uint64); t_del uint64 | None.  Returns a dict: pos_set uint32, old_pos int32, K, V, and val_ptr /
    values (lists) or dates.  Two items that name one position: the slice is kept when ANY of them is alive (the tests let them agree)."""
    t_set, pos_set, t_unset = words
    p = pos_set.astype(np.int64) - 1
    valid = (p >= 0) & (p < n_events)
    win = np.unique(p[valid])
    k = int(win.size)
    out_pos = np.zeros(n_items, np.uint32)
    out_pos[valid] = np.searchsorted(win, p[valid]) + 1
    res = dict(pos_set=out_pos, old_pos=win.astype(np.int32), K=k, V=0)
    if vp is not None:
        n_values = int(vals.size)
        alive = P.alive_np(t_set, t_unset, t_del if t_del is not None else np.zeros(n_items, np.uint64))
        alive_pos = np.zeros(k, bool)
        np.logical_or.at(alive_pos, out_pos[valid].astype(np.int64) - 1, alive[valid])
        lo = np.maximum(vp[win], 0)
        hi = np.maximum(np.minimum(vp[win + 1], n_values), lo)
        ln = np.where(alive_pos, np.minimum(hi - lo, I32_MAX), 0)
        out_vp = np.minimum(np.concatenate([[0], np.cumsum(ln)]), n_values).astype(np.int64)
        take = np.diff(out_vp)
        res["val_ptr"] = out_vp
        res["values"] = np.concatenate([vals[a:a + t] for a, t in zip(lo, take)] + [np.zeros(0, np.int32)]).astype(np.int32)
        res["V"] = int(out_vp[-1])
    if dates is not None:
        res["dates"] = dates[win]
    return res


def _words(st: PC.DevState):
    return st.words()


def _t_del_words(t_del):
    return t_del.cpu().numpy().view(np.uint64).copy() if t_del is not None else None


def run_compact(sess, st: PC.DevState, t_del, vp=None, vals=None, dates=None, sizes=(0, 0), pad=0):
    """One urcco_dev_props_compact call through ctypes, the outputs at exactly sizes = (K, V) entries (K + 1 for out_val_ptr; one where that is 0) plus
    `pad`, filled with the sentinel.  Returns (status, dict of the outputs whole, counts)."""
    n, (k, v) = st.n_items, sizes
    o = dict(pos_set=sess.empty(max(n, 1) + pad, torch.int32), old_pos=sess.empty(max(k, 1) + pad, torch.int32))
    if vp is not None:
        o["val_ptr"], o["values"] = sess.empty(k + 1 + pad, torch.int64), sess.empty(max(v, 1) + pad, torch.int32)
    if dates is not None:
        o["dates"] = sess.empty(max(k, 1) + pad, torch.int64)
    for t in o.values():
        t.fill_(SENTINEL)
    counts = sess.empty(2, torch.int64)
    counts.fill_(SENTINEL)
    d_vp = put(sess, vp) if vp is not None else None
    d_vals = put(sess, vals) if vp is not None and vals.size else None
    d_dates = (put(sess, dates) if dates.size else sess.empty(1, torch.int64)) if dates is not None else None
    state = st.struct(t_del)
    ptr = lambda name: o[name].data_ptr() if name in o else None      # noqa: E731
    status = sess.lib.urcco_dev_props_compact(sess.handle, n, C.byref(state), d_vp.data_ptr() if d_vp is not None else None, d_vals.data_ptr() if d_vals is not None else None,
                                              int(vals.size) if vp is not None else 0, d_dates.data_ptr() if d_dates is not None else None, ptr("pos_set"), ptr("old_pos"),
                                              ptr("val_ptr"), ptr("values"), ptr("dates"), counts.data_ptr())
    sess.synchronize()
    return status, {name: t.cpu().numpy() for name, t in o.items()}, counts.cpu().numpy()


def stream_arrays(p: PC.Prop, n_events):
    """(val_ptr, values, None) of a list property's first n_events positions, (None, None, dates) of a date property's"""
    if p.lists is None:
        return None, None, p.dates[:n_events]
    vp, vals = PC.value_arrays(p)
    return vp[: n_events + 1], vals[: vp[n_events]], None


def check_call(sess, name, st: PC.DevState, t_del, vp, vals, dates, pad=3):
    """The call against the restatement, and the sentinel behind every output.  Returns the restatement's dict."""
    n = st.n_items
    before = (_words(st), _t_del_words(t_del))
    want = compact_ref(n, before[0], before[1], st.n_events, vp, vals, dates)
    k, v = want["K"], want["V"]
    status, got, counts = run_compact(sess, st, t_del, vp, vals, dates, (k, v), pad)
    assert status == _lib.OK, name
    assert counts.tolist() == [k, v], (name, counts, k, v)
    assert np.array_equal(got["pos_set"][:n].view(np.uint32), want["pos_set"]), name
    assert np.array_equal(got["old_pos"][:k], want["old_pos"]), name
    assert (got["pos_set"][max(n, 1):] == SENTINEL).all() and (got["old_pos"][max(k, 1):] == SENTINEL).all() and (k > 0 or got["old_pos"][0] == SENTINEL), f"{name}: written at or past out_old_pos[K]"
    if vp is not None:
        assert np.array_equal(got["val_ptr"][: k + 1], want["val_ptr"]), (name, got["val_ptr"][:8], want["val_ptr"][:8])
        assert np.array_equal(got["values"][:v], want["values"]), name
        assert (got["val_ptr"][k + 1:] == SENTINEL).all(), f"{name}: written at or past out_val_ptr[K + 1]"
        assert (got["values"][max(v, 1):] == SENTINEL).all() and (v > 0 or got["values"][0] == SENTINEL), f"{name}: written at or past out_values[V]"
    if dates is not None:
        assert np.array_equal(got["dates"][:k], want["dates"]), name
        assert (got["dates"][max(k, 1):] == SENTINEL).all() and (k > 0 or got["dates"][0] == SENTINEL), f"{name}: written at or past out_date_values[K]"
    after = (_words(st), _t_del_words(t_del))
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and (before[1] is None or np.array_equal(before[1], after[1])), f"{name}: the state was written"
    return want


def compacted(sess, st: PC.DevState, p: PC.Prop, want):
    """(the state, the Prop) of the compacted stream, from the restatement's outputs: what a caller that swaps the outputs in holds"""
    k = want["K"]
    new = PC.DevState(sess, st.n_items)
    new.t_set, new.t_unset, new.n_events = st.t_set, st.t_unset, k
    if st.n_items:
        new.pos_set.copy_(torch.from_numpy(want["pos_set"].view(np.int32).copy()))
    old = want["old_pos"].astype(np.int64)
    kinds = p.kinds_or_set()[old]
    if p.lists is not None:
        vp = want["val_ptr"]
        q = PC.Prop(p.items[old], p.times[old], kinds, [want["values"][vp[j]:vp[j + 1]].tolist() for j in range(k)], None, p.n_cols)
    else:
        q = PC.Prop(p.items[old], p.times[old], kinds, None, want["dates"], 0)
    return new, q


def check_prop(sess, name, n_items, p: PC.Prop, t_del=None, st=None, pad=3):
    """One property: the call against the restatement; then _bounds / _rows (or _dates) and _exists over the compacted stream == over the stream as it
    was.  Returns (the compacted state, the compacted Prop, the restatement's dict)."""
    st = st if st is not None else PC.apply_in(sess, n_items, p, [0, p.n])
    vp, vals, dates = stream_arrays(p, st.n_events)
    want = check_call(sess, name, st, t_del, vp, vals, dates, pad)
    new, q = compacted(sess, st, p, want)
    if p.lists is not None:
        a, b = PC.run_rows(sess, st, t_del, p), PC.run_rows(sess, new, t_del, q)
        assert np.array_equal(a[0], b[0]), f"{name}: the bounds differ"
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3][: a[2][-1]], b[3][: b[2][-1]]), f"{name}: the rows differ"
    else:
        assert np.array_equal(PC.run_dates(sess, st, t_del, p), PC.run_dates(sess, new, t_del, q)), f"{name}: the dates differ"
    if t_del is not None and n_items:
        assert np.array_equal(PC.run_exists(sess, n_items, t_del, [st.t_set]), PC.run_exists(sess, n_items, t_del, [new.t_set])), name
    return new, q, want


# ---- kernel-level cases ---------------------------------------------------------------------------------------------------------------------------
def slice_cases(sess, n_cols=3000):
    """winner slices of 0, 1, 63, 64, 65, 4096, 4097 and 8193 values among superseded, unset and never-set items"""
    rng = np.random.default_rng(7)
    lists = PC.edge_lists(rng, n_cols)
    n_items = len(lists) + 3                                  # the last three: never set, unset later, superseded by a short list
    ev = [(i, T0 + i, SET) for i in range(len(lists))] + [(n_items - 2, T0, SET), (n_items - 2, T0 + 1, UNSET), (n_items - 1, T0, SET), (n_items - 1, T0 + 1, SET)]
    all_lists = lists + [rng.integers(0, n_cols, 100).tolist(), [], rng.integers(0, n_cols, 5000).tolist(), [4, 2]]
    for seed in (1, 2):
        order = np.random.default_rng(seed).permutation(len(ev))
        p = PC.prop([ev[j] for j in order], lists=[all_lists[j] for j in order], n_cols=n_cols)
        _, _, want = check_prop(sess, f"slices {seed}", n_items, p)
        assert sorted(np.diff(want["val_ptr"]).tolist()) == sorted([len(l) for l in lists] + [0, 2])      # the unset item's winner keeps its position, with an empty slice
        assert want["K"] == len(lists) + 2 and want["V"] == sum(len(l) for l in lists) + 2 < sum(len(l) for l in all_lists) - 5000


def _constant(name):
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "universal-recommender_amd", "csrc", "cco_props.h")).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


def tile_cases(sess):
    """the copy's tiles: one-value winners (a tile touches exactly PC_TILE of them, staged in LDS) and one-value winners among dead ones (a tile touches
    more winners than the staging holds: the search in global memory)"""
    tile, lds = _constant("PC_TILE"), _constant("PC_LDS")
    rng = np.random.default_rng(13)
    n_items = 3 * tile + 5
    for dead in (0.0, 0.6):
        ev = [(i, T0, SET) for i in range(n_items)]
        lists = [[int(i % 50)] for i in range(n_items)]
        gone = np.flatnonzero(rng.random(n_items) < dead)
        ev += [(int(i), T0 + 1, UNSET) for i in gone]
        lists += [[] for _ in gone]
        order = rng.permutation(len(ev))
        p = PC.prop([ev[j] for j in order], lists=[lists[j] for j in order], n_cols=50)
        _, _, want = check_prop(sess, f"tiles dead={dead}", n_items, p)
        vp = want["val_ptr"]
        spans = [int(np.searchsorted(vp, min(e + tile, want["V"]) - 1, side="right") - np.searchsorted(vp, e, side="right")) + 1 for e in range(0, want["V"], tile)]
        assert want["K"] == n_items and want["V"] == n_items - gone.size and len(spans) >= 2
        assert (max(spans) > lds) == (dead > 0) and (dead > 0 or max(spans) == tile), spans


def owner_case(sess, n_hot=100_000, n_rest=100):
    """one item owns n_hot of the n_hot + n_rest events"""
    rng = np.random.default_rng(8)
    n, n_items = n_hot + n_rest, 50
    items = np.full(n, 17, np.int32)
    items[rng.choice(n, n_rest, replace=False)] = rng.integers(0, n_items, n_rest).astype(np.int32)
    times = (T0 + rng.permutation(n) // 3).astype(np.int64)
    kinds = (rng.random(n) < 0.4).astype(np.uint8)
    lists = [[] if k else [int(j % 11), int(j % 7)] for j, k in enumerate(kinds)]
    t_del = PC.run_delete(sess, n_items, np.full(3, 16, np.int32), np.array([T0, T0 + 5, T0 + 2], np.int64))
    _, _, want = check_prop(sess, "owner", n_items, PC.Prop(items, times, kinds, lists, None, 11), t_del)
    assert 1 < want["K"] <= n_items and want["V"] <= 2 * want["K"]
    dates = rng.integers(-5, 10**12, n).astype(np.int64)
    check_prop(sess, "owner dates", n_items, PC.Prop(items, times, kinds, None, dates, 0), t_del)


def dead_case(sess):
    """every winner is dead: V == 0, K positions with empty slices, and the store answers as before"""
    rng = np.random.default_rng(11)
    n_items, n = 70, 600
    p = PC.random_prop(rng, n_items, n, 9, unset=0.0, stray=False)
    late = PC.prop([(i, T0 + 100, UNSET) for i in range(0, n_items, 2)], lists=[[] for _ in range(0, n_items, 2)], n_cols=9)
    p = PC.Prop(np.concatenate([p.items, late.items]), np.concatenate([p.times, late.times]), np.concatenate([p.kinds, late.kinds]), p.lists + late.lists, None, 9)
    t_del = PC.run_delete(sess, n_items, np.arange(1, n_items, 2).astype(np.int32), np.full(n_items // 2, T0 + 100, np.int64))
    _, _, want = check_prop(sess, "dead", n_items, p, t_del)
    assert want["V"] == 0 and want["K"] == np.unique(p.items[: n]).size > 60 and not want["val_ptr"].any()


def domain_cases(sess):
    """n_items of 0, 1, 63, 64 and 65; n_events == 0; a zero-extended state"""
    rng = np.random.default_rng(12)
    for n_items in (0, 1, 63, 64, 65):
        n = 5 * n_items + 40
        check_prop(sess, f"n_items {n_items}", n_items, PC.random_prop(rng, n_items, n, 7))
        check_prop(sess, f"n_items {n_items} dates", n_items, PC.random_prop(rng, n_items, n, 0, date=True))
        t_del = PC.run_delete(sess, n_items, rng.integers(0, max(n_items, 1), 9).astype(np.int32), rng.integers(T0, T0 + 50, 9).astype(np.int64)) if n_items else None
        check_prop(sess, f"n_items {n_items} deletes", n_items, PC.random_prop(rng, n_items, n, 7), t_del)
    for n_items in (0, 5):                                               # no events: K = V = 0, out_val_ptr = [0]
        empty = PC.prop([], lists=[], n_cols=3)
        _, _, want = check_prop(sess, f"no events {n_items}", n_items, empty)
        assert want["K"] == 0 and want["val_ptr"].tolist() == [0]
        check_prop(sess, f"no events {n_items} dates", n_items, PC.prop([], dates=[]))
    n0, n1, n = 40, 70, 400                                              # the catalogue grew: the new items name no position
    p = PC.random_prop(rng, n0, n, 6)
    st = PC.apply_in(sess, n0, p, [0, n]).grown(n1)
    _, _, want = check_prop(sess, "grown", n1, p, st=st)
    assert not want["pos_set"][n0:].any() and 0 < want["K"] <= n0


def malformed_cases(sess):
    """pos_set beyond the stream, two items naming one position, val_ptr entries outside the value array: the result may be wrong, no access leaves
    the arrays (HIPSIM_GUARD; the outputs have exactly K, K + 1 and V entries)"""
    p = PC.prop([(0, T0, SET), (1, T0, SET), (2, T0, SET), (3, T0, SET), (4, T0, SET)], lists=[[1, 2], [3], [0, 1, 2, 3], [], [6, 5]], n_cols=7)
    vp, vals, _ = stream_arrays(p, 5)
    for pos in ([9, 2, -1, 1, 0], [3, 3, 3, 3, 3], [0, 0, 0, 0, 0], [6, 7, I32_MAX, -(1 << 31), -2], [5, 1, 5, 1, 2]):
        st = PC.apply_in(sess, 5, p, [0, 5])
        st.pos_set.copy_(torch.tensor(pos, dtype=torch.int32))
        want = check_call(sess, f"pos_set {pos}", st, None, vp, vals, None)
        assert want["K"] == len({x for x in pos if 1 <= x <= 5})
        check_call(sess, f"pos_set {pos} dates", st, None, None, None, np.arange(5, dtype=np.int64))
    st = PC.apply_in(sess, 5, p, [0, 5])
    values = np.arange(9, dtype=np.int32)
    for bad in ([0, -5, 3, 99, 4, 9], [0, 9, 2, 7, 1, 8], [5, 4, 3, 2, 1, 0], [I64_MIN, I64_MAX, I64_MIN, I64_MAX, 0, I64_MAX], [0, 9, 0, 9, 0, 9], [0, 0, 9, 9, 9, 9]):
        want = check_call(sess, f"val_ptr {bad}", st, None, np.array(bad, np.int64), values, None)
        assert 0 <= want["V"] <= 9 and want["K"] == 5
    # a stream longer than the state knows (n_events below the arrays' length is the caller's statement): positions at and beyond it name nothing
    st.n_events = 3
    want = check_call(sess, "short n_events", st, None, vp[:4], vals[: vp[3]], None)
    assert want["K"] == 3 and want["pos_set"].tolist() == [1, 2, 3, 0, 0]


def bad_argument_cases(sess):
    lib, h = sess.lib, sess.handle
    n = 4
    st = PC.DevState(sess, n)
    st.n_events = 3
    st.pos_set.copy_(torch.tensor([1, 3, 0, 2], dtype=torch.int32))
    td = PC.zeros(sess, n, torch.int64)
    vp, vals, dv = put(sess, np.arange(4, dtype=np.int64)), put(sess, np.zeros(3, np.int32)), put(sess, np.zeros(3, np.int64))
    o_ps, o_op, o_vp, o_v, o_d, cnt = (sess.empty(n, torch.int32), sess.empty(3, torch.int32), sess.empty(4, torch.int64), sess.empty(3, torch.int32),
                                       sess.empty(3, torch.int64), sess.empty(2, torch.int64))
    BAD, OK = _lib.BAD_ARG, _lib.OK

    def state(**kw):
        s = st.struct(td)
        for k, v in kw.items():
            setattr(s, k, v)
        return C.byref(s)
    ok = dict(s=h, n=n, state=state(), vp=vp.data_ptr(), vals=vals.data_ptr(), nv=3, dv=None, o_ps=o_ps.data_ptr(), o_op=o_op.data_ptr(), o_vp=o_vp.data_ptr(),
              o_v=o_v.data_ptr(), o_d=None, cnt=cnt.data_ptr())

    def call(**kw):
        a = dict(ok, **kw)
        return lib.urcco_dev_props_compact(a["s"], a["n"], a["state"], a["vp"], a["vals"], a["nv"], a["dv"], a["o_ps"], a["o_op"], a["o_vp"], a["o_v"], a["o_d"], a["cnt"])

    dates = dict(vp=None, vals=None, nv=0, dv=dv.data_ptr(), o_vp=None, o_v=None, o_d=o_d.data_ptr())
    assert call() == OK and call(**dates) == OK
    assert call(state=state(t_del=None)) == OK
    assert call(vp=None, vals=None, nv=0, o_vp=None, o_v=None) == OK                                   # neither lists nor dates: the positions alone
    sess.synchronize()
    assert cnt.tolist() == [3, 0] and o_ps.tolist() == [1, 3, 0, 2]
    for b in (None, state(t_set=None), state(pos_set=None), state(t_unset=None), state(n_events=-1), state(n_events=1 << 31)):      # the state's refusals
        assert call(state=b) == BAD
    assert call(s=None) == BAD and call(n=-1) == BAD and call(nv=-1) == BAD
    assert call(dv=dv.data_ptr(), o_d=o_d.data_ptr()) == BAD                                           # lists and dates together
    for name in ("o_ps", "o_op", "o_vp", "vals", "o_v", "cnt"):                                        # a NULL the call needs
        assert call(**{name: None}) == BAD, name
    assert call(**dict(dates, o_d=None)) == BAD and call(**dict(dates, o_op=None)) == BAD
    # NULLs the call does not need
    assert call(nv=0, vals=None, o_v=None) == OK
    assert call(n=0, state=state(t_set=None, pos_set=None, t_unset=None, t_del=None), o_ps=None, o_op=None, vals=None, o_v=None) == OK
    assert call(state=state(n_events=0), o_op=None, vals=None, o_v=None) == OK
    sess.synchronize()
    assert cnt.tolist() == [0, 0] and int(o_vp[0]) == 0 and o_ps.tolist() == [0, 0, 0, 0]
    assert lib.urcco_version() == 305


# ---- the store, a compacted one and its uncompacted twin ------------------------------------------------------------------------------------------
class Model:
    """what DeviceProperties reads of a model: the size of the primary's dictionary, dense integer ids"""

    def __init__(self, sess, n_items):
        self.sess, self.n_items = sess, n_items


def snapshot(dp):
    """every output of a store as numpy: the matrices (row_ptr, col_idx, col_ptr), the dates, the mask, and t_set / t_unset / t_del"""
    props, dates = dp.materialise()
    out = {f"{name}.{f}": getattr(p, f).cpu().numpy() for name, p in props.items() for f in ("row_ptr", "col_idx", "col_ptr")}
    out.update({f"{name}.n_cols": np.array([p.n_cols]) for name, p in props.items()})
    out.update({f"date {name}": d.cpu().numpy() for name, d in dates.items()})
    out["mask"] = dp.item_mask().cpu().numpy()
    out["t_del"] = dp.t_del.cpu().numpy()
    for name, s in dp.streams.items():
        out[f"{name}.t_set"], out[f"{name}.t_unset"] = s.t_set.cpu().numpy(), s.t_unset.cpu().numpy()
    return out


def same(a, b):
    return a.keys() == b.keys() and all(x.dtype == b[k].dtype and np.array_equal(x, b[k]) for k, x in a.items())


def check_stream_shape(dp):
    """n_events is the length every stream array is read at, and the state names positions inside it"""
    for s in dp.streams.values():
        k = s.n_events
        assert all(getattr(s, a).numel() >= k for a in ("items", "times", "kinds") if getattr(s, a) is not None)
        pos = s.pos_set.cpu().numpy().view(np.uint32)[: dp.n_items]
        assert pos.max(initial=0) <= k
        if not s.is_date and s.val_ptr is not None:
            vp = s.val_ptr.cpu().numpy()[: k + 1]
            assert vp[0] == 0 and vp[-1] == s.n_values and (np.diff(vp) >= 0).all()
        items, times = s.items.cpu().numpy()[:k], s.times.cpu().numpy()[:k]
        named = np.flatnonzero(pos)
        assert np.array_equal(items[pos[named].astype(np.int64) - 1], named)                     # the gathered streams follow the positions
        assert np.array_equal(times[pos[named].astype(np.int64) - 1].view(np.uint64) ^ np.uint64(1 << 63), s.t_set.cpu().numpy().view(np.uint64)[named])


def twin_case(sess):
    """7 batches into three stores: one never compacted, one compacted between every two batches, one compacted once in the middle.  After every batch
    all three agree in every output.  Batch 4 holds, for items whose winner's time is known from the batches before: a $set at exactly that time (the
    later position wins the tie), an $unset at that time, a $delete at that time, and the unset that batch 5's later $set revives."""
    from universal_recommender_amd.properties import DeviceProperties
    rng = np.random.default_rng(21)
    n_items, n_cols = 90, 12
    values = [f"v{j}" for j in range(n_cols)]

    def batch(n, planted=()):
        out = {}
        for name, date in (("cat", False), ("tag", False), ("day", True)):
            p = PC.random_prop(rng, n_items, n, n_cols, t_hi=T0 + 40, date=date)
            ev = [e for e in planted if e[0] == name]
            items = np.concatenate([p.items, np.array([e[1] for e in ev], np.int32)])
            times = np.concatenate([p.times, np.array([e[2] for e in ev], np.int64)])
            kinds = np.concatenate([p.kinds, np.array([e[3] for e in ev], np.uint8)])
            if date:
                payload = np.concatenate([p.dates, np.arange(len(ev), dtype=np.int64) + 777])
            else:
                lists = p.lists + [([3, 1] if e[3] == SET else []) for e in ev]
                vp = np.zeros(len(lists) + 1, np.int64)
                np.cumsum([len(x) for x in lists], out=vp[1:])
                payload = (vp, np.array([v for x in lists for v in x], np.int32))
            out[name] = (items, times, kinds, payload)
        return out

    stores = {mode: DeviceProperties(sess, Model(sess, n_items), ["day"]) for mode in ("never", "always", "once")}
    for dp in stores.values():
        dp.apply_streams({}, new_values={"cat": values, "tag": values})
    seen = {"cat": ([], [], [])}
    before_compaction = None
    for k in range(7):
        planted, deletes = [], (rng.integers(0, n_items, 4).astype(np.int32), rng.integers(T0, T0 + 40, 4).astype(np.int64))
        if k in (4, 5):
            t_set, _, t_unset = P.aggregate_np(n_items, *[np.concatenate(x) for x in seen["cat"]])
            when = lambda i: int(t_set[i] ^ np.uint64(1 << 63))      # noqa: E731 -- the winner's time of item i, as a signed time
            assert all(t_set[i] > t_unset[i] for i in (0, 1, 2)) or k == 5
            if k == 4:
                planted = [("cat", 0, when(0), SET), ("cat", 1, when(1), UNSET), ("cat", 3, when(3) + 1, UNSET), ("day", 0, T0 + 39, SET)]
                deletes = (np.array([2], np.int32), np.array([when(2)], np.int64))
                revive_at = when(3) + 2
            else:
                planted = [("cat", 3, revive_at, SET)]
        b = batch(150 + 40 * k, planted)
        if k < 4:                                                    # items 0 .. 3 hold an alive winner when batch 4 arrives
            for i in range(4):
                b["cat"][0][i], b["cat"][1][i], b["cat"][2][i] = i, T0 + 45 + k, SET
            deletes = (deletes[0] + 4, deletes[1])
        for a, x in zip(seen["cat"], b["cat"][:3]):
            a.append(x)
        for mode, dp in stores.items():
            assert dp.apply_streams(b, deletes) is dp
        shots = {mode: snapshot(dp) for mode, dp in stores.items()}
        assert same(shots["never"], shots["always"]) and same(shots["never"], shots["once"]), k
        if k == 4:                                                   # the planted events did what they are there for
            rp = shots["never"]["cat.row_ptr"]
            ci = shots["never"]["cat.col_idx"]
            assert ci[rp[0]:rp[1]].tolist() == [1, 3] and rp[2] == rp[1] and rp[3] == rp[2] and rp[4] == rp[3] and shots["never"]["mask"][2] == 0
        if k == 5:
            rp = shots["never"]["cat.row_ptr"]
            assert shots["never"]["cat.col_idx"][rp[3]:rp[4]].tolist() == [1, 3]      # revived
        for mode, dp in stores.items():
            if mode == "always" or (mode == "once" and k == 3):
                n_before = {name: (s.n_events, s.n_values) for name, s in dp.streams.items()}
                cap_before = {name: (s.items.numel(), s.val_ptr.numel() if s.val_ptr is not None else 0) for name, s in dp.streams.items()}
                assert dp.compact() is dp
                assert set(dp.last_compact) == set(dp.streams)
                for name, s in dp.streams.items():
                    e0, e1, v0, v1 = dp.last_compact[name]
                    assert (e0, v0) == n_before[name] and (e1, v1) == (s.n_events, s.n_values) and e1 <= min(e0, n_items) and v1 <= v0
                    assert (s.items.numel(), s.val_ptr.numel() if s.val_ptr is not None else 0) == cap_before[name]      # the capacity stays, as spare
                assert any(e1 < e0 for e0, e1, _, _ in dp.last_compact.values())
                check_stream_shape(dp)
                assert same(snapshot(dp), shots["never"]), (mode, k)
    assert stores["always"].streams["cat"].n_events <= n_items + 190 + 40 * 6 < stores["never"].streams["cat"].n_events
    # names: one property alone; a name the store does not hold
    dp = stores["never"]
    want = snapshot(dp)
    n_tag = dp.streams["tag"].n_events
    dp.compact(["cat"])
    assert set(dp.last_compact) == {"cat"} and dp.streams["tag"].n_events == n_tag and dp.streams["cat"].n_events <= n_items and same(snapshot(dp), want)
    try:
        dp.compact(["no such property"])
    except ValueError:
        pass
    else:
        raise AssertionError("compact of an unknown name did not raise")
    # a grown catalogue, then events for the new items, on a compacted store
    for dp in (stores["always"], stores["once"]):
        dp.grow(n_items + 7)
    late = {"cat": (np.array([n_items + 3, 5], np.int32), np.array([T0, T0 + 99], np.int64), None, (np.array([0, 1, 3], np.int64), np.array([2, 4, 5], np.int32)))}
    shots = [snapshot(dp.apply_streams(late).compact()) for dp in (stores["always"], stores["once"])]
    assert same(*shots) and shots[0]["cat.row_ptr"].size == n_items + 8


def predict_case(sess):
    """set_properties + batch_predict with rules, before and after a compaction: the golden stack of tests/test_props_predict.py after its inventory change"""
    from test_props_predict import _answers, _bare, _property_map
    from test_recommend_rules_golden import DAY_MS, NOW_MS, _iso, _render, _stack
    from universal_recommender_amd.properties import DeviceProperties
    algo, model, docs, history, items, doc, dates, props = _stack(sess)
    queries = [_render(q["query"]) for q in doc["queries"]]
    wide = [{k: v for k, v in q.items() if k not in ("num", "from")} | {"num": model.n_items} for q in queries]
    dp = DeviceProperties.from_property_map(sess, model, _property_map(doc, dates, props), algo.dateNames)
    dp.apply([("Nexus", "$set", {"categories": ["Phones", "Electronics", "Google", "Refurbished"]}, 10), ("Iphone 4", "$unset", ["countries"], 10), ("Galaxy", "$delete", None, 10),
              ("Ipad-retina", "$set", {"expires": _iso(NOW_MS + 30 * DAY_MS)}, 11), ("Surface", "$set", {"categories": ["Phones"]}, 12)])
    m = _bare(model).set_properties(dp)
    mask = dp.item_mask()
    before = (_answers(algo, m, queries, history, mask), _answers(algo, m, wide, history, mask), snapshot(dp))
    n_before = {name: s.n_events for name, s in dp.streams.items()}
    assert dp.compact() is dp and any(s.n_events < n_before[name] for name, s in dp.streams.items())
    m2 = _bare(model).set_properties(dp)
    mask2 = dp.item_mask()
    assert torch.equal(mask, mask2) and same(snapshot(dp), before[2])
    assert _answers(algo, m2, queries, history, mask2) == before[0] and _answers(algo, m2, wide, history, mask2) == before[1]
    assert any(s["score"] > 0 for r in before[1] for s in r["itemScores"])
    # and on: an event after the compaction is answered as on the uncompacted twin
    dp.apply([("Nexus", "$unset", ["categories"], 13)])
    m3 = _bare(model).set_properties(dp)
    assert _answers(algo, m3, wide, history, dp.item_mask()) != before[1]


# ---- the larger shape (GPU) -----------------------------------------------------------------------------------------------------------------------
def larger_shape_case(sess):
    """D25's larger shape -- 2^20 + 77 property events over 2^16 items, Zipf(1.2), a third of them $unsets, 500 $deletes, two list properties and one
    date, three batches -- compacted: the outputs against the restatement, and every output of the store as before"""
    from universal_recommender_amd.properties import DeviceProperties
    rng = np.random.default_rng(47)
    n, n_items = (1 << 20) + 77, 1 << 16
    sizes = {"categories": (n - 2 * (n // 4), 900), "tags": (n // 4, 70_000), "expires": (n // 4, 0)}
    dp = DeviceProperties(sess, Model(sess, n_items), ["expires"])
    dp.apply_streams({}, new_values={name: [f"v{j}" for j in range(c)] for name, (_, c) in sizes.items() if c})
    host = {}
    for name, (m, n_cols) in sizes.items():
        items = ((rng.zipf(1.2, m) - 1) % n_items).astype(np.int32)
        items[rng.integers(0, m, 200)] = np.array([-1, n_items, PC.I32_MIN, PC.I32_MAX], np.int32)[rng.integers(0, 4, 200)]
        times = (T0 + rng.integers(0, 5000, m)).astype(np.int64)
        kinds = (rng.random(m) < 1 / 3).astype(np.uint8)
        if n_cols:
            lens = np.where(kinds == SET, rng.integers(0, 5, m), 0)
            long = rng.choice(np.flatnonzero(kinds == SET), 3, replace=False)
            lens[long], items[long], times[long] = [70, 8193, 4097], [1000, 1001, 1002], T0 + 6000
            vp = np.zeros(m + 1, np.int64)
            np.cumsum(lens, out=vp[1:])
            payload = (vp, rng.integers(-1, n_cols + 1, int(vp[-1])).astype(np.int32))
        else:
            payload = rng.integers(-10**9, 10**13, m).astype(np.int64)
        host[name] = (items, times, kinds, payload)
    d_items, d_times = rng.integers(-1, n_items + 1, 500).astype(np.int32), (T0 + rng.integers(0, 5000, 500)).astype(np.int64)
    d_items[:100] = np.arange(100)
    for lo, hi in ((0.0, 0.45), (0.45, 0.45), (0.45, 1.0)):
        b = {}
        for name, (items, times, kinds, payload) in host.items():
            a, z = int(lo * items.size), int(hi * items.size)
            part = payload[a:z] if sizes[name][1] == 0 else (payload[0][a:z + 1] - payload[0][a], payload[1][payload[0][a]:payload[0][z]])
            b[name] = (items[a:z], times[a:z], kinds[a:z], part)
        a, z = int(lo * 500), int(hi * 500)
        dp.apply_streams(b, (d_items[a:z], d_times[a:z]))
    before = snapshot(dp)
    t_del = P.delete_np(n_items, d_items, d_times)
    want = {}
    for name, (items, times, kinds, payload) in host.items():
        words = P.aggregate_np(n_items, items, times, kinds)
        want[name] = compact_ref(n_items, words, t_del, items.size, *((payload[0], payload[1], None) if sizes[name][1] else (None, None, payload)))
    assert dp.compact() is dp
    for name, s in dp.streams.items():
        w = want[name]
        k, v = w["K"], w["V"]
        assert dp.last_compact[name] == (host[name][0].size, k, int(host[name][3][0][-1]) if sizes[name][1] else 0, v), name
        assert 1000 < k < n_items and (s.n_events, s.n_values) == (k, v)
        assert np.array_equal(s.pos_set.cpu().numpy().view(np.uint32)[:n_items], w["pos_set"]), name
        assert np.array_equal(s.items.cpu().numpy()[:k], host[name][0][w["old_pos"]]) and np.array_equal(s.times.cpu().numpy()[:k], host[name][1][w["old_pos"]]), name
        if sizes[name][1]:
            assert np.array_equal(s.val_ptr.cpu().numpy()[: k + 1], w["val_ptr"]) and np.array_equal(s.vals.cpu().numpy()[:v], w["values"]), name
            assert np.diff(w["val_ptr"]).max() == 8193
        else:
            assert np.array_equal(s.date_vals.cpu().numpy()[:k], w["dates"]), name
    assert same(snapshot(dp), before)
