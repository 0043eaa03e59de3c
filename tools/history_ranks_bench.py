#!/usr/bin/env python3
"""Times urcco_dev_history_ranks and urcco_dev_fill_order (decision D24) against the other route to the same backfill order that exists without them --
urcco_dev_pop_counts over the same stream with the ids already mapped to items, then the torch.sort of DeviceModel.from_indicators -- on the GPU: HIP
events around windows of --inner calls, warm, several repetitions; times are per call.  All outputs are allocated beforehand; no call synchronises.

Shape: one timed stream of --events events whose items follow a Zipf(1.1) distribution over --items columns, times uniform over an hour; the window is
that hour.  The stream is counted twice: with its columns being the items (straight into the item table) and through a column map (a permutation:
counted in the column space, folded per column).  The counts of both must equal those of urcco_dev_pop_counts bit for bit, and the one-field order must
equal the torch.sort order.  Printed beside the times: the bytes of the decision's cost model and the GB/s they give over the best time --
  counting   12 B per event (item 4, time 8); per item 4 B per interval cleared and 4 B read, 8 B of rank written; with a column map per column 4 B per
             interval cleared and read and 4 B of map (the atomics of the table and of the fold are not in the count)
  order      per field 16 B per item for the smallest key and the differing bits, 20 B per item for the keys (id 4, rank 8, key 8), and per pass 8 B
             (histogram) + 24 B (key and id read and written) per item; 4 B for the identity, 8 B for the result
usage: tools/history_ranks_bench.py [--events N] [--items N] [--reps N] [--inner N] [--log FILE]"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from universal_recommender_amd import _lib  # noqa: E402
from universal_recommender_amd.device import DeviceSession  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--events", type=int, default=1 << 24)
ap.add_argument("--items", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=10, help="calls per timed window; the printed times are per call")
ap.add_argument("--log", default=None, help="also write the lines to this file")
args = ap.parse_args()

assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
dev = torch.device("cuda", 0)
sess = DeviceSession(dev, _lib.load(os.environ.get("URCCO_LIB", _lib.DEFAULT_PATH)))
lines = []
NONE = _lib.RANK_NONE
T0, HOUR = 1_600_000_000_000, 3_600_000


def say(line):
    print(line, flush=True)
    lines.append(line)


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / args.inner)
    return ms


def show(ms):
    return f"{min(ms):.3f} ms best, {sorted(ms)[len(ms) // 2]:.3f} ms median of {len(ms)} (spread {max(ms) - min(ms):.3f}; {[round(x, 3) for x in ms]})"


check = lambda status: _lib.check(status, sess.lib)  # noqa: E731
rng = np.random.default_rng(43)
n, n_items = args.events, args.items
cols = torch.from_numpy(((rng.zipf(1.1, n) - 1) % n_items).astype(np.int32)).to(dev)
times = torch.from_numpy((T0 + rng.integers(0, HOUR, n)).astype(np.int64)).to(dev)
cmap = torch.from_numpy(rng.permutation(n_items).astype(np.int32)).to(dev)
mapped = cmap[cols.long()].contiguous()      # the other route's ids: mapped outside the timed window
say(f"stream: {n} events, items Zipf(1.1) over {n_items} columns (the hottest takes {int(torch.bincount(cols).max())}), times uniform over an hour, the window is that hour")

rank = {k: sess.empty(n_items, torch.int64) for k in ("popular", "trending", "hot")}
counts = sess.empty(3 * n_items, torch.int32)
ref_counts = sess.empty(3 * n_items, torch.int32)
types = {"popular": _lib.RANK_POPULAR, "trending": _lib.RANK_TRENDING, "hot": _lib.RANK_HOT}


def ranks_call(kind, with_map, want_counts=False):
    st = (_lib.RankStream * 1)(_lib.RankStream(n, cols.data_ptr(), times.data_ptr(), cmap.data_ptr() if with_map else None, n_items, 0))
    return lambda: check(sess.lib.urcco_dev_history_ranks(sess.handle, st, 1, n_items, types[kind], T0, T0 + HOUR, rank[kind].data_ptr(),
                                                          counts.data_ptr() if want_counts else None))


def pop_call(kind, ids):
    k = types[kind]
    step = HOUR // k
    b = (C.c_int64 * (k + 1))(*([T0 + j * step for j in range(k)] + [T0 + HOUR]))
    return lambda: check(sess.lib.urcco_dev_pop_counts(sess.handle, n, ids.data_ptr(), times.data_ptr(), n_items, k, b, ref_counts.data_ptr()))


for kind in ("popular", "hot"):
    k = types[kind]
    for with_map, ids, what in ((False, cols, "columns are items"), (True, mapped, "through a column map")):
        ranks_call(kind, with_map, True)()
        pop_call(kind, ids)()
        torch.cuda.synchronize()
        assert torch.equal(counts[: k * n_items], ref_counts[: k * n_items]), "the two routes disagree on the counts"
        ms_r, ms_p = timed(ranks_call(kind, with_map), args.reps), timed(pop_call(kind, ids), args.reps)
        n_bytes = 12 * n + (8 * k + 8) * n_items + ((8 * k + 4) * n_items if with_map else 0)
        say(f"{kind}, {what}: urcco_dev_history_ranks {show(ms_r)}")
        say(f"    urcco_dev_pop_counts over the same stream, ids mapped beforehand (counts only, no ranks): {show(ms_p)}")
        say(f"    bytes by the decision's count: 12 x {n} + {8 * k + 8} x {n_items}" + (f" + {8 * k + 4} x {n_items}" if with_map else "") +
            f" = {n_bytes}; over the best time: {n_bytes / (min(ms_r) * 1e-3) / 1e9:.1f} GB/s")
ranks_call("trending", False)()
torch.cuda.synchronize()


def passes(fields):
    out = []
    for f in fields:
        v = f.cpu().numpy()
        raw = v.astype(np.uint64) ^ np.uint64(1 << 63)
        has = v != NONE
        key = np.where(has, raw - (raw[has].min() if has.any() else np.uint64(0)) + np.uint64(1), np.uint64(0))      # the distance from the field's smallest key (csrc/cco_ranks.h)
        d = int(np.bitwise_or.reduce(key ^ key[0]))
        out.append(sum(((d >> (8 * b)) & 255) != 0 for b in range(8)))
    return out


order = sess.empty(n_items, torch.int32)
for name, fields in (("one field (popular)", [rank["popular"]]), ("three fields (hot, trending, popular)", [rank["hot"], rank["trending"], rank["popular"]])):
    ptrs = (C.c_void_p * len(fields))(*[f.data_ptr() for f in fields])
    call = lambda: check(sess.lib.urcco_dev_fill_order(sess.handle, n_items, ptrs, len(fields), order.data_ptr()))  # noqa: E731
    ms = timed(call, args.reps)
    p = passes(fields)
    n_bytes = n_items * (12 + 36 * len(fields) + 32 * sum(p))
    say(f"urcco_dev_fill_order, {name}, {n_items} items, passes per field {p}: {show(ms)}")
    say(f"    bytes by the decision's count: {n_items} x (12 + 36 x {len(fields)} + 32 x {sum(p)}) = {n_bytes}; over the best time: {n_bytes / (min(ms) * 1e-3) / 1e9:.1f} GB/s")
    if len(fields) == 1:
        r = torch.where(fields[0] == NONE, torch.full((), float("-inf"), dtype=torch.float64, device=dev), fields[0].to(torch.float64))
        sort_call = lambda: torch.sort(-r, stable=True).indices.to(torch.int32)  # noqa: E731
        ms_t = timed(sort_call, args.reps)
        assert torch.equal(sort_call(), order), "the two routes disagree on the order"
        say(f"    torch.sort(-rank as float64, stable) of DeviceModel.from_indicators, ranks already on the device: {show(ms_t)}")
say(f"{int((rank['popular'] != NONE).sum())} / {int((rank['trending'] != NONE).sum())} / {int((rank['hot'] != NONE).sum())} of {n_items} items have a popular / trending / hot rank")
say(f"one run on one MI355X, HIP events around {args.inner} calls per window (times per call), two warm-up calls before the windows; no alternation of the routes, no repeat on "
    "another box; the inputs of every call are those of the call before and stay in the caches")
if args.log:
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
sess.close()
