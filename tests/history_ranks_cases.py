"""urcco_dev_history_ranks / urcco_dev_fill_order (decision D24 of DESIGN.md, include/urcco.h): the problems and checks that tests/test_sim_history_ranks.py
and tests/test_gpu_history_ranks.py share.  The contract, restated in numpy (counts_ref, ranks_ref, fill_ref):

    D = t_end - t_start, step = D // type;  bounds = [t_start + k * step for k < type] + [t_end]            (type: popular 1, trending 2, hot 3)
    in_b[p]   = times is None ? b == 0 : bounds[b] <= times[p] and (times[p] < bounds[b + 1] or (b == type - 1 and t_end == INT64_MAX))
    item[p]   = c = items[p] in 0 .. n_cols ? (col_map ? col_map[c] : c) : none;  counted when in 0 .. n_items
    counts[b][i] = the counted positions of all streams with item i in interval b
    rank[i]   = c0 if popular, c1 - c0 if trending, (c2 - c1) - (c1 - c0) if hot -- when every count it joins is > 0, else NONE
    order     = lexsort by (key of field 0, key of field 1, ..., item id), key = NONE ? 0 : uint64(value) ^ 2^63, descending in every key

Every array goes to the device in a tensor of exactly its size and every output is allocated at exactly its size plus `pad` sentinel entries: a read or
write past either end faults under HIPSIM_GUARD, and check asserts that the padding still holds the sentinel."""
import ctypes as C
import os
import re
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import history_ref as H
from history_append_cases import put
from universal_recommender_amd import _lib

I64_MIN, I64_MAX = H.I64_MIN, H.I64_MAX
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
NONE = _lib.RANK_NONE
SENTINEL = H.SENTINEL
T0 = 1_600_000_000_000
POPULAR, TRENDING, HOT = _lib.RANK_POPULAR, _lib.RANK_TRENDING, _lib.RANK_HOT
OPEN = (I64_MIN, I64_MAX)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile():
    text = open(os.path.join(ROOT, "universal-recommender_amd", "csrc", "cco_kernels.h")).read()
    return int(re.search(r"constexpr int RK_TILE = (\d+);", text).group(1))


TILE = _tile()      # pairs one block of the sort places per pass (csrc/cco_kernels.h RK_TILE)


@dataclass
class RStream:
    items: np.ndarray                 # int32 [n_events]
    times: Optional[np.ndarray]       # int64 [n_events] or None
    col_map: Optional[np.ndarray]     # int32 [n_cols] or None
    n_cols: int


# ---- the contract in numpy ------------------------------------------------------------------------------------------------------------------------
def bounds_ref(rtype, t_start, t_end):
    step = (t_end - t_start) // rtype
    return [t_start + k * step for k in range(rtype)] + [t_end]


def counts_ref(streams, n_items, rtype, t_start, t_end):
    b = bounds_ref(rtype, t_start, t_end)
    counts = np.zeros((rtype, n_items), np.int64)
    for s in streams:
        c = s.items.astype(np.int64)
        ok = (c >= 0) & (c < s.n_cols)
        i = np.where(ok, c, 0)
        if s.col_map is not None:
            i = s.col_map.astype(np.int64)[i] if s.n_cols else i
        ok &= (i >= 0) & (i < n_items)
        for k in range(rtype):
            if s.times is None:
                inb = np.full(c.size, k == 0)
            else:
                inb = (s.times >= b[k]) & ((s.times < b[k + 1]) | (k == rtype - 1 and t_end == I64_MAX))
            np.add.at(counts[k], i[ok & inb], 1)
    return counts


def ranks_ref(counts):
    c = counts.astype(np.int64)
    r = c[0] if len(c) == 1 else (c[1] - c[0] if len(c) == 2 else (c[2] - c[1]) - (c[1] - c[0]))
    return np.where((c > 0).all(axis=0), r, NONE).astype(np.int64)


def fill_ref(fields, n):
    keys = [~np.where(v == NONE, np.uint64(0), v.astype(np.uint64) ^ np.uint64(1 << 63)) for v in fields]
    return np.lexsort([np.arange(n)] + keys[::-1]).astype(np.int32)


# ---- the calls ------------------------------------------------------------------------------------------------------------------------------------
def _stream_arg(sess, s: RStream, keep):
    n = int(s.items.size)
    d_items = put(sess, s.items) if n else sess.empty(1, torch.int32)            # a stream of no events still has one-element buffers
    d_times = None if s.times is None else (put(sess, s.times) if n else sess.empty(1, torch.int64))
    d_map = None if s.col_map is None else (put(sess, s.col_map) if s.col_map.size else sess.empty(1, torch.int32))
    keep += [d_items, d_times, d_map]
    return _lib.RankStream(n, d_items.data_ptr(), d_times.data_ptr() if d_times is not None else None, d_map.data_ptr() if d_map is not None else None, s.n_cols, 0)


def run_ranks(sess, streams, n_items, rtype, t_start, t_end, want_counts=True, pad=0):
    """One urcco_dev_history_ranks call through ctypes: (status, rank [max(n_items, 1) + pad], counts [max(type * n_items, 1) + pad] | None)"""
    keep = []
    arr = (_lib.RankStream * max(len(streams), 1))(*[_stream_arg(sess, s, keep) for s in streams])
    rank = sess.empty(max(n_items, 1) + pad, torch.int64)
    rank.fill_(SENTINEL)
    cnt = None
    if want_counts:
        cnt = sess.empty(max(rtype * n_items, 1) + pad, torch.int32)
        cnt.fill_(SENTINEL)
    status = sess.lib.urcco_dev_history_ranks(sess.handle, arr, len(streams), n_items, rtype, t_start, t_end, rank.data_ptr(), cnt.data_ptr() if cnt is not None else None)
    sess.synchronize()
    return status, rank.cpu().numpy(), cnt.cpu().numpy() if cnt is not None else None


def check_ranks(sess, name, streams, n_items, rtype, window, want_counts=True, pad=0):
    w_counts = counts_ref(streams, n_items, rtype, *window)
    w_rank = ranks_ref(w_counts)
    status, rank, cnt = run_ranks(sess, streams, n_items, rtype, window[0], window[1], want_counts, pad)
    assert status == _lib.OK, (name, rtype, window)
    assert np.array_equal(rank[:n_items], w_rank), (name, rtype, window, rank[:n_items][:20], w_rank[:20])
    assert (rank[max(n_items, 1):] == SENTINEL).all(), f"{name}: written at or past out_rank[n_items]"
    if want_counts:
        assert np.array_equal(cnt[: rtype * n_items].reshape(rtype, n_items), w_counts), (name, rtype, window)
        assert (cnt[max(rtype * n_items, 1):] == SENTINEL).all(), f"{name}: written at or past out_counts[type * n_items]"
    return w_rank, w_counts


def run_fill(sess, fields, n, pad=0, same=()):
    """One urcco_dev_fill_order call through ctypes: (status, order [max(n, 1) + pad]).  same: pairs (f, g) -- field f is passed as the pointer of field g"""
    d = [put(sess, np.ascontiguousarray(v, np.int64)) if n else sess.empty(1, torch.int64) for v in fields]
    for f, g in same:
        d[f] = d[g]
    ptrs = (C.c_void_p * max(len(d), 1))(*[t.data_ptr() for t in d])
    out = sess.empty(max(n, 1) + pad, torch.int32)
    out.fill_(SENTINEL)
    status = sess.lib.urcco_dev_fill_order(sess.handle, n, ptrs, len(d), out.data_ptr())
    sess.synchronize()
    return status, out.cpu().numpy()


def check_fill(sess, name, fields, n, pad=0, same=()):
    fields = [np.asarray(v, np.int64) for v in fields]
    for f, g in same:
        assert np.array_equal(fields[f], fields[g])
    want = fill_ref(fields, n)
    status, out = run_fill(sess, fields, n, pad, same)
    assert status == _lib.OK, name
    assert np.array_equal(np.sort(out[:n]), np.arange(n)), f"{name}: not a permutation"
    assert np.array_equal(out[:n], want), (name, out[:n][:20], want[:20])
    assert (out[max(n, 1):] == SENTINEL).all(), f"{name}: written at or past out_order[n_items]"
    return want


# ---- counting: the interval bounds ----------------------------------------------------------------------------------------------------------------
def boundary_times(rtype, t_start, t_end):
    """t_start - 1, t_start, each inner bound - 1 / bound / bound + 1, t_end - 1, t_end"""
    b = bounds_ref(rtype, t_start, t_end)
    out = [t_start - 1, t_start, t_end - 1, t_end] + [x + d for x in b[1:-1] for d in (-1, 0, 1)]
    return np.array(sorted({t for t in out if I64_MIN <= t <= I64_MAX}), np.int64)


def window_stream(rng, times_of, n_items, n=600):
    return RStream(rng.integers(0, n_items, n).astype(np.int32), times_of[rng.integers(0, times_of.size, n)], None, n_items)


def boundary_cases(sess):
    rng = np.random.default_rng(5)
    n_items = 9
    for d in (1001, 1000, 7, 6, 3):          # 1001: divisible by neither 2 nor 3; 7 likewise; 6 by both
        for rtype in (POPULAR, TRENDING, HOT):
            t = boundary_times(rtype, T0, T0 + d)
            s = window_stream(rng, t, n_items)
            rank, counts = check_ranks(sess, f"bounds D={d}", [s], n_items, rtype, (T0, T0 + d), pad=3)
            b = bounds_ref(rtype, T0, T0 + d)
            for k in range(rtype):          # start inclusive, end exclusive: exactly the events with b[k] <= t < b[k + 1]
                assert counts[k].sum() == int(((s.times >= b[k]) & (s.times < b[k + 1])).sum()) > 0
            assert counts.sum() < s.items.size and (rank != NONE).any()
    # one item per interval pattern: the joins
    items = np.array([0] * 3 + [1] * 2 + [2] * 1 + [3] * 5 + [4] * 3, np.int32)
    times = T0 + np.array([0, 30, 60] + [0, 30] + [60] + [0, 30, 60, 61, 62] + [0, 1, 60], np.int64)      # D = 90: thirds at 30, 60; halves at 45
    s = RStream(items, times, None, 6)
    assert check_ranks(sess, "joins", [s], 6, POPULAR, (T0, T0 + 90))[0].tolist() == [3, 2, 1, 5, 3, NONE]
    assert check_ranks(sess, "joins", [s], 6, TRENDING, (T0, T0 + 90))[0].tolist() == [-1, NONE, NONE, 1, -1, NONE]
    assert check_ranks(sess, "joins", [s], 6, HOT, (T0, T0 + 90))[0].tolist() == [0, NONE, NONE, 2, NONE, NONE]
    # D = 0: nothing; D = 1 and D = 2: D // 3 == 0, the older and the middle interval of hot are empty
    t = np.array([T0 - 1, T0, T0 + 1, T0 + 2], np.int64)
    s = window_stream(rng, t, n_items, 200)
    for rtype in (POPULAR, TRENDING, HOT):
        assert (check_ranks(sess, "D=0", [s], n_items, rtype, (T0, T0))[0] == NONE).all()
        for d in (1, 2):
            rank, counts = check_ranks(sess, f"D={d}", [s], n_items, rtype, (T0, T0 + d))
            if rtype == HOT:
                assert (rank == NONE).all() and counts[0].sum() == 0 and counts[1].sum() == 0 and counts[2].sum() > 0
    assert (check_ranks(sess, "D=1", [s], n_items, TRENDING, (T0, T0 + 1))[0] == NONE).all()      # D // 2 == 0
    assert (check_ranks(sess, "D=2", [s], n_items, TRENDING, (T0, T0 + 2))[0] != NONE).any()


def open_window_cases(sess):
    rng = np.random.default_rng(7)
    n_items = 5
    t = np.array([I64_MIN, I64_MIN + 1, -1, 0, T0, I64_MAX - 1, I64_MAX], np.int64)
    s = window_stream(rng, t, n_items, 300)
    rank, counts = check_ranks(sess, "open", [s], n_items, POPULAR, OPEN)
    assert counts.sum() == 300                                               # INT64_MIN and INT64_MAX - 1 (and INT64_MAX: no end) are inside
    for rtype in (POPULAR, TRENDING, HOT):                                   # t_end == INT64_MAX: the last interval has no end
        rank, counts = check_ranks(sess, "no end", [s], n_items, rtype, (0, I64_MAX))
        assert counts[-1].sum() >= int((s.times >= I64_MAX - 1).sum()) > 0 and counts.sum() == int((s.times >= 0).sum())
        _, counts = check_ranks(sess, "end", [s], n_items, rtype, (0, I64_MAX - 1))
        assert counts.sum() == int(((s.times >= 0) & (s.times < I64_MAX - 1)).sum())
    check_ranks(sess, "from the start", [s], n_items, POPULAR, (I64_MIN, 0))
    check_ranks(sess, "negative", [s], n_items, HOT, (I64_MIN, I64_MIN + 10))


# ---- counting: ids, column maps, streams ----------------------------------------------------------------------------------------------------------
def id_cases(sess):
    rng = np.random.default_rng(11)
    n_cols, n_items, n = 12, 8, 500
    hostile = np.array([-1, n_cols, I32_MIN, I32_MAX], np.int32)
    items = np.where(rng.random(n) < 0.2, hostile[rng.integers(0, 4, n)], rng.integers(0, n_cols, n)).astype(np.int32)
    assert set(hostile.tolist()) <= set(items.tolist())
    times = (T0 + rng.integers(0, 90, n)).astype(np.int64)
    cmap = np.array([3, -1, 0, 3, n_items, 7, I32_MAX, 1, 1, I32_MIN, 5, 2], np.int32)      # -1, >= n_items, two pairs of columns on one item
    assert cmap.size == n_cols
    win = (T0, T0 + 90)
    for rtype in (POPULAR, TRENDING, HOT):
        _, c_map = check_ranks(sess, "col_map", [RStream(items, times, cmap, n_cols)], n_items, rtype, win, pad=2)
        assert c_map[:, 3].sum() == int(np.isin(items, (0, 3)).sum()) and c_map[:, 4].sum() == 0 and c_map[:, 6].sum() == 0      # the merged columns add
        _, c_wide = check_ranks(sess, "identity, n_cols > n_items", [RStream(items, times, None, n_cols)], n_items, rtype, win)
        assert c_wide.sum() == int(((items >= 0) & (items < n_items)).sum())                                                         # ids beyond n_items dropped
        _, c_narrow = check_ranks(sess, "identity, n_cols < n_items", [RStream(items, times, None, 5)], n_items, rtype, win)
        assert c_narrow[:, 5:].sum() == 0 and c_narrow.sum() == int(((items >= 0) & (items < 5)).sum())
    check_ranks(sess, "n_cols 0", [RStream(items, times, None, 0)], n_items, POPULAR, win)
    check_ranks(sess, "n_cols 0, mapped", [RStream(items, times, np.zeros(0, np.int32), 0)], n_items, POPULAR, win)


def stream_cases(sess):
    rng = np.random.default_rng(13)
    n_items = 10
    mk = lambda n, n_cols, timed: RStream(rng.integers(-1, n_cols + 1, n).astype(np.int32), (T0 + rng.integers(0, 300, n)).astype(np.int64) if timed else None, None, n_cols)      # noqa: E731
    a, b, c = mk(400, n_items, True), mk(300, 7, False), mk(350, 14, True)
    c.col_map = rng.integers(-1, n_items, 14).astype(np.int32)
    _, counts = check_ranks(sess, "three streams, one untimed", [a, b, c], n_items, POPULAR, OPEN, pad=1)
    assert counts.sum() == sum(int(counts_ref([s], n_items, POPULAR, *OPEN).sum()) for s in (a, b, c))
    empty = RStream(np.zeros(0, np.int32), np.zeros(0, np.int64), None, n_items)
    empty_mapped = RStream(np.zeros(0, np.int32), np.zeros(0, np.int64), c.col_map, 14)
    win = (T0, T0 + 300)
    for rtype in (POPULAR, TRENDING, HOT):
        _, once = check_ranks(sess, "one stream", [c], n_items, rtype, win)
        _, twice = check_ranks(sess, "one stream twice", [c, c], n_items, rtype, win)
        assert np.array_equal(twice, 2 * once) and once.sum() > 0
        check_ranks(sess, "timed streams", [a, c, empty, a, empty_mapped], n_items, rtype, win)
        assert (check_ranks(sess, "an empty stream", [empty], n_items, rtype, win)[0] == NONE).all()
        assert (check_ranks(sess, "no stream", [], n_items, rtype, win)[0] == NONE).all()
        rank, _ = check_ranks(sess, "one item", [a], 1, rtype, win, pad=4)
        assert rank.size == 1
        check_ranks(sess, "no counts wanted", [a, c], n_items, rtype, win, want_counts=False, pad=2)
        assert run_ranks(sess, [a], 0, rtype, win[0], win[1])[0] == _lib.OK      # no item: nothing is written
    check_ranks(sess, "sixteen streams", [a] * _lib.RANK_MAX_STREAMS, n_items, HOT, win)


def cache_cases(sess):
    """70 000 events on one item: the block cache's flush carries every count; 70 000 over 5 000 items (up to 15 000 keys with three intervals): keys that
    miss both probes of a block's cache go to the table directly.  Both over a col_map, and straight into the item table."""
    rng = np.random.default_rng(17)
    n = 70_000
    times = (T0 + rng.integers(0, 900, n)).astype(np.int64)
    for name, n_cols, items in (("one item", 40, np.full(n, 17, np.int32)), ("5000 items", 5000, rng.integers(0, 5000, n).astype(np.int32))):
        cmap = rng.permutation(n_cols).astype(np.int32)
        for rtype in (POPULAR, HOT):
            _, counts = check_ranks(sess, name, [RStream(items, times, None, n_cols)], n_cols, rtype, (T0, T0 + 900))
            assert counts.sum() == n and (counts.max() > 20_000 if n_cols == 40 else np.count_nonzero(counts) > 4096)
            check_ranks(sess, name + ", mapped", [RStream(items, times, cmap, n_cols)], n_cols, rtype, (T0, T0 + 900))


def rank_bad_argument_cases(sess):
    lib = sess.lib
    n_items, n = 6, 50
    rng = np.random.default_rng(19)
    d_items, d_times = put(sess, rng.integers(0, n_items, n).astype(np.int32)), put(sess, (T0 + rng.integers(0, 90, n)).astype(np.int64))
    d_map = put(sess, np.arange(n_items, dtype=np.int32))
    rank, cnt = sess.empty(n_items, torch.int64), sess.empty(3 * n_items, torch.int32)

    def call(streams=None, n_streams=None, **kw):
        a = dict(s=sess.handle, n_items=n_items, type=HOT, lo=T0, hi=T0 + 90, rank=rank.data_ptr(), cnt=cnt.data_ptr())
        a.update(kw)
        streams = [dict()] if streams is None else streams
        arr = (_lib.RankStream * max(len(streams), 1))()
        for k, st in enumerate(streams):
            v = dict(n=n, items=d_items.data_ptr(), times=d_times.data_ptr(), map=None, n_cols=n_items)
            v.update(st)
            arr[k] = _lib.RankStream(v["n"], v["items"], v["times"], v["map"], v["n_cols"], 0)
        return lib.urcco_dev_history_ranks(a["s"], arr if n_streams != "null" else None, len(streams) if n_streams in (None, "null") else n_streams, a["n_items"], a["type"],
                                           a["lo"], a["hi"], a["rank"], a["cnt"])

    assert call() == _lib.OK and call(cnt=None) == _lib.OK
    assert call(type=0) == _lib.BAD_ARG and call(type=4) == _lib.BAD_ARG and call(type=-1) == _lib.BAD_ARG
    assert call(n_streams=-1) == _lib.BAD_ARG and call([dict()] * 17) == _lib.BAD_ARG and call(n_streams="null") == _lib.BAD_ARG
    assert call([dict()] * 16) == _lib.OK and call([]) == _lib.OK
    assert call(lo=T0 + 1, hi=T0) == _lib.BAD_ARG and call(lo=T0, hi=T0) == _lib.OK
    for rtype in (TRENDING, HOT):                                              # D beyond 64 bits
        assert call(type=rtype, lo=-2, hi=I64_MAX - 1) == _lib.BAD_ARG and call(type=rtype, lo=I64_MIN, hi=0) == _lib.BAD_ARG
        assert call(type=rtype, lo=I64_MIN, hi=I64_MAX) == _lib.BAD_ARG and call(type=rtype, lo=0, hi=I64_MAX) == _lib.OK and call(type=rtype, lo=-1, hi=I64_MAX - 1) == _lib.OK
    assert call(type=POPULAR, lo=-2, hi=I64_MAX - 1) == _lib.OK and call(type=POPULAR, lo=I64_MIN, hi=I64_MAX) == _lib.OK
    # a stream without times: only popular over the open window
    assert call([dict(times=None)]) == _lib.BAD_ARG and call([dict(times=None)], type=POPULAR) == _lib.BAD_ARG
    assert call([dict(times=None)], type=POPULAR, lo=I64_MIN, hi=I64_MAX - 1) == _lib.BAD_ARG and call([dict(times=None)], type=POPULAR, lo=I64_MIN + 1, hi=I64_MAX) == _lib.BAD_ARG
    assert call([dict(), dict(times=None)], type=POPULAR, lo=I64_MIN, hi=I64_MAX) == _lib.OK
    assert call([dict(n=0, times=None)]) == _lib.BAD_ARG
    # 32-bit counts: the events of all streams together
    assert call([dict(n=1 << 30), dict(n=1 << 30)]) == _lib.BAD_ARG and call([dict(n=I32_MAX), dict(n=1)]) == _lib.BAD_ARG and call([dict(n=1 << 62)] * 2) == _lib.BAD_ARG
    assert call(n_items=0x7ffffff0 // 3 + 1) == _lib.BAD_ARG and call([dict(map=d_map.data_ptr(), n_cols=0x7ffffff0 // 3 + 1)]) == _lib.BAD_ARG
    assert call(n_items=-1) == _lib.BAD_ARG and call([dict(n=-1)]) == _lib.BAD_ARG and call([dict(n_cols=-1)]) == _lib.BAD_ARG
    assert call([dict(items=None)]) == _lib.BAD_ARG and call([dict(n=0, items=None)]) == _lib.OK
    assert call(rank=None) == _lib.BAD_ARG and call(rank=None, n_items=0) == _lib.OK and call(s=None) == _lib.BAD_ARG
    assert call([dict(map=d_map.data_ptr())]) == _lib.OK
    sess.synchronize()
    assert lib.urcco_version() == 305


# ---- the fill order -------------------------------------------------------------------------------------------------------------------------------
FILL_SIZES = (0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)
SPECIALS = np.array([I64_MIN + 1, -1, 0, 1, I64_MAX, NONE], np.int64)


def fill_size_cases(sess):
    rng = np.random.default_rng(23)
    for n in FILL_SIZES:
        counts = rng.integers(1, 40, n).astype(np.int64)
        counts[rng.random(n) < 0.3] = NONE
        check_fill(sess, f"counts n={n}", [counts], n, pad=3)
        check_fill(sess, f"all NONE n={n}", [np.full(n, NONE)], n)
        check_fill(sess, f"all equal n={n}", [np.full(n, 12345)], n)
        check_fill(sess, f"all distinct n={n}", [rng.permutation(n).astype(np.int64) - n // 2], n)
        check_fill(sess, f"specials n={n}", [SPECIALS[rng.integers(0, SPECIALS.size, n)]], n, pad=1)
        check_fill(sess, f"two fields n={n}", [rng.integers(0, 3, n), SPECIALS[rng.integers(0, SPECIALS.size, n)]], n)
    want = check_fill(sess, "specials, each once", [SPECIALS], SPECIALS.size)
    assert want.tolist() == [4, 3, 2, 1, 0, 5]      # INT64_MAX first, INT64_MIN + 1 last of the ranks, NONE behind it
    assert check_fill(sess, "identity", [], 777, pad=2).tolist() == list(range(777))      # n_fields == 0
    assert run_fill(sess, [], 0)[0] == _lib.OK


def fill_digit_cases(sess):
    """keys that differ in one byte only: every other digit takes no pass; in the lowest and the top byte together: two passes, six skipped between"""
    rng = np.random.default_rng(29)
    n = TILE + 300
    base = 0x0123456789ABCDEF
    for name, shifts in (("top byte", (56,)), ("lowest byte", (0,)), ("byte 3", (24,)), ("lowest and top", (0, 56)), ("bytes 1, 2, 6", (8, 16, 48))):
        v = np.full(n, base, np.int64)
        for sh in shifts:
            v = v ^ (rng.integers(0, 256, n).astype(np.int64) << np.int64(sh))
        d = np.bitwise_or.reduce(v ^ v[0])
        assert all(((int(d) >> (8 * b)) & 255 != 0) == (8 * b in shifts) for b in range(8)), name
        want = check_fill(sess, name, [v], n)
        assert (np.unique(v).size < n or len(shifts) > 1) and (v[want][:-1] >= v[want][1:]).all()
    # top byte: the sign bit flips the order of the two halves
    v = (rng.integers(0, 256, n).astype(np.int64) << np.int64(56)) | np.int64(5)
    want = check_fill(sess, "sign byte", [v], n)
    assert v[want[0]] == v.max() > 0 > v.min() == v[want[-1]]


def fill_stability_cases(sess):
    """ten distinct values over three tiles: equal values keep ascending item ids across the tile borders; fields whose earlier ones tie heavily"""
    rng = np.random.default_rng(31)
    n = 3 * TILE
    v = rng.integers(0, 10, n).astype(np.int64) * 1000
    want = check_fill(sess, "ten values", [v], n, pad=2)
    for x in np.unique(v):
        ids = want[v[want] == x]
        assert (np.diff(ids) > 0).all() and ids[0] < TILE and ids[-1] >= 2 * TILE
    n = 2 * TILE + 77
    f = [rng.integers(0, 2, n), rng.integers(0, 3, n), np.where(rng.random(n) < 0.5, NONE, rng.integers(-2, 3, n)), rng.integers(0, 1 << 40, n)]
    for k in (2, 3, 4):
        want = check_fill(sess, f"{k} fields", f[:k], n)
        assert (np.diff(np.asarray(f[0])[want]) <= 0).all()
    check_fill(sess, "heavy ties, last decides", [np.zeros(n, np.int64), np.full(n, NONE), np.ones(n, np.int64), f[3]], n)
    check_fill(sess, "one pointer twice", [f[1], f[3], f[1]], n, same=((2, 0),))
    check_fill(sess, "one pointer in every field", [f[2]] * 4, n, same=((1, 0), (2, 0), (3, 0)))
    v = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)      # the whole int64 domain: eight passes
    v[:5] = (NONE, I64_MIN + 1, I64_MAX, 0, -1)
    check_fill(sess, "full domain", [v], n)
    check_fill(sess, "full domain, two fields", [rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True) >> np.int64(62), v], n)


def fill_bad_argument_cases(sess):
    lib = sess.lib
    n = 100
    d = put(sess, np.arange(n, dtype=np.int64))
    out = sess.empty(n, torch.int32)
    ptrs = lambda *p: (C.c_void_p * max(len(p), 1))(*p)      # noqa: E731
    ok = ptrs(d.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr())
    for k in range(5):
        assert lib.urcco_dev_fill_order(sess.handle, n, ok, k, out.data_ptr()) == _lib.OK
    assert lib.urcco_dev_fill_order(sess.handle, n, ok, 5, out.data_ptr()) == _lib.BAD_ARG and lib.urcco_dev_fill_order(sess.handle, n, ok, -1, out.data_ptr()) == _lib.BAD_ARG
    assert lib.urcco_dev_fill_order(sess.handle, n, ptrs(d.data_ptr(), None), 2, out.data_ptr()) == _lib.BAD_ARG      # a NULL field
    assert lib.urcco_dev_fill_order(sess.handle, n, None, 1, out.data_ptr()) == _lib.BAD_ARG and lib.urcco_dev_fill_order(sess.handle, n, None, 0, out.data_ptr()) == _lib.OK
    assert lib.urcco_dev_fill_order(sess.handle, n, ok, 1, None) == _lib.BAD_ARG and lib.urcco_dev_fill_order(sess.handle, 0, ok, 1, None) == _lib.OK
    assert lib.urcco_dev_fill_order(sess.handle, -1, ok, 1, out.data_ptr()) == _lib.BAD_ARG and lib.urcco_dev_fill_order(None, n, ok, 1, out.data_ptr()) == _lib.BAD_ARG
    sess.synchronize()


def from_indicators_case(sess):
    """one field == the order DeviceModel.from_indicators(ranks=dict) builds for the same values: rank desc, items without a rank last, then item index"""
    from helpers import rand_csr, run_device
    from oracle import c_oracle as O
    from universal_recommender_amd.recommend import DeviceModel
    rng = np.random.default_rng(37)
    n_items = 150
    out = run_device(sess, [rand_csr(rng, 300, n_items, 8)], [O.DatasetParams(100, 20, None)], 7)
    v = rng.integers(-3, 9, n_items).astype(np.int64)      # heavy ties, negative ranks (trending)
    v[rng.random(n_items) < 0.3] = NONE
    as_dict = {i: float(x) for i, x in enumerate(v.tolist()) if x != NONE}
    want = DeviceModel.from_indicators(sess, [("purchase", out[0])], ranks=as_dict).fill_order
    model = DeviceModel.from_indicators(sess, [("purchase", out[0])])
    assert model.fill_order is None and model.rank_fields == {}
    got = model.set_ranks({"popRank": put(sess, v)}).fill_order
    sess.synchronize()
    assert want.dtype == got.dtype == torch.int32 and torch.equal(got.cpu(), want.cpu()) and np.array_equal(want.cpu().numpy(), fill_ref([v], n_items))
    assert model.rank_fields["popRank"].dtype == torch.int64 and model.set_ranks({}).fill_order is None and model.rank_fields == {}
