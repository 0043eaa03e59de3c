"""The aggregation rule of the device-resident item properties (decision D25 of DESIGN.md, include/urcco.h urcco_dev_props_*), restated in plain Python over
a list of events -- the reference tests/props_cases.py checks the device against -- and once more in numpy for shapes the loop is too slow for.

Per item i and property p, over all events seen so far:
    S        the $set of (i, p) with the largest (time, stream position)
    U, D     the largest time of an $unset of (i, p); the largest time of a $delete of i
    alive    S exists and time(S) > U and time(S) > D
    value    that of S alone
    deleted  a $delete of i exists and no property of i has a set later than D
An event with time INT64_MIN, an item outside 0 .. n_items or a kind other than SET / UNSET is ignored."""
import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SET, UNSET = 0, 1


def bias(t: int) -> int:
    """the state's word for a time: (uint64)t ^ 2^63"""
    return (int(t) + (1 << 63)) & ((1 << 64) - 1)


def aggregate(n_items, events):
    """events: (item, time, kind) per stream position of ONE property.  Returns (S: item -> (time, position), U: item -> time)"""
    S, U = {}, {}
    for p, (i, t, k) in enumerate(events):
        i, t, k = int(i), int(t), int(k)
        if not 0 <= i < n_items or t == I64_MIN:
            continue
        if k == SET:
            if i not in S or (t, p) > S[i]:
                S[i] = (t, p)
        elif k == UNSET:
            if i not in U or t > U[i]:
                U[i] = t
    return S, U


def aggregate_deletes(n_items, deletes):
    """deletes: (item, time) per $delete.  Returns D: item -> time"""
    D = {}
    for i, t in deletes:
        i, t = int(i), int(t)
        if 0 <= i < n_items and t != I64_MIN and (i not in D or t > D[i]):
            D[i] = t
    return D


def state_words(n_items, S, U):
    """(t_set uint64, pos_set uint32, t_unset uint64): the state arrays the device holds for (S, U)"""
    t_set, pos_set, t_unset = np.zeros(n_items, np.uint64), np.zeros(n_items, np.uint32), np.zeros(n_items, np.uint64)
    for i, (t, p) in S.items():
        t_set[i], pos_set[i] = bias(t), p + 1
    for i, t in U.items():
        t_unset[i] = bias(t)
    return t_set, pos_set, t_unset


def delete_words(n_items, D):
    t_del = np.zeros(n_items, np.uint64)
    for i, t in D.items():
        t_del[i] = bias(t)
    return t_del


def alive(S, U, D, i) -> bool:
    return i in S and (i not in U or S[i][0] > U[i]) and (i not in D or S[i][0] > D[i])


def winners(n_items, S, U, D):
    """item -> stream position of S, for the items whose property is alive"""
    return {i: S[i][1] for i in range(n_items) if alive(S, U, D, i)}


def exists_mask(n_items, sets, D):
    """sets: the S of every property.  uint8 [n_items]: 0 iff the item is deleted"""
    m = np.ones(n_items, np.uint8)
    for i, d in D.items():
        if not any(i in S and S[i][0] > d for S in sets):
            m[i] = 0
    return m


def rows_of(n_items, win, lists, n_cols):
    """The item x value matrix of the alive winners: (row_ptr int64, col_idx int32, pairs) -- lists[p] = the value ids of stream position p; ids outside
    0 .. n_cols have no column; pairs = the (item, value id) pairs of the alive winners, those ids dropped, as two int32 arrays."""
    rows = [sorted({int(v) for v in lists[win[i]] if 0 <= int(v) < n_cols}) if i in win else [] for i in range(n_items)]
    rp = np.zeros(n_items + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    pr = np.array([i for i in range(n_items) if i in win for v in lists[win[i]] if 0 <= int(v) < n_cols], np.int32)
    pc = np.array([int(v) for i in range(n_items) if i in win for v in lists[win[i]] if 0 <= int(v) < n_cols], np.int32)
    return rp, np.array([v for r in rows for v in r], np.int32), (pr, pc)


def dates_of(n_items, win, date_values):
    out = np.full(n_items, I64_MIN, np.int64)
    for i, p in win.items():
        out[i] = date_values[p]
    return out


def aggregated_map(n_items, item_name, props, D):
    """The aggregated dict item name -> {property: value} a host rebuild starts from.  props: name -> (S, U, values per stream position)"""
    out = {}
    for name, (S, U, values) in props.items():
        for i, p in winners(n_items, S, U, D).items():
            out.setdefault(item_name(i), {})[name] = values[p]
    return out


# ---- the same in numpy (tests/test_gpu_props.py: a million events) ----------------------------------------------------------------------------------
def _u(t):
    return t.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)


def aggregate_np(n_items, items, times, kinds):
    """state words (t_set, pos_set, t_unset) of one property's stream"""
    items, times, kinds = np.asarray(items, np.int64), np.asarray(times, np.int64), np.asarray(kinds)
    ok = (items >= 0) & (items < n_items) & (times != I64_MIN)
    bt = _u(times)
    t_set, pos_set, t_unset = np.zeros(n_items, np.uint64), np.zeros(n_items, np.uint32), np.zeros(n_items, np.uint64)
    s = np.flatnonzero(ok & (kinds == SET))
    np.maximum.at(t_set, items[s], bt[s])
    top = s[bt[s] == t_set[items[s]]]
    np.maximum.at(pos_set, items[top], (top + 1).astype(np.uint32))
    u = np.flatnonzero(ok & (kinds == UNSET))
    np.maximum.at(t_unset, items[u], bt[u])
    return t_set, pos_set, t_unset


def delete_np(n_items, items, times):
    items, times = np.asarray(items, np.int64), np.asarray(times, np.int64)
    ok = (items >= 0) & (items < n_items) & (times != I64_MIN)
    t_del = np.zeros(n_items, np.uint64)
    np.maximum.at(t_del, items[ok], _u(times[ok]))
    return t_del


def alive_np(t_set, t_unset, t_del):
    return (t_set != 0) & (t_set > t_unset) & (t_set > t_del)


def exists_np(t_sets, t_del):
    later = np.zeros(t_del.size, bool)
    for t in t_sets:
        later |= t > t_del
    return ((t_del == 0) | later).astype(np.uint8)
