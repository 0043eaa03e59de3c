#!/usr/bin/env python3
"""Times urcco_dev_history_cap (decision D27) on the GPU against (a) the only other route to the same state -- the cap decided on the host over numpy
copies of the stream (a lexsort by user, time, position), the filtered arrays copied to the device and urcco_dev_history_index over the filtered `users`:
what DeviceHistory.from_streams over host-filtered streams does -- and (b) urcco_dev_history_trim with the time rule alone on the same stream, the floor
of the pipeline the two calls share.  HIP events around windows of --inner calls for the two library calls, warm, several repetitions, times per call;
wall-clock around device synchronisations for the host route, whose parts are printed separately (the host filter; the copies and the index).

Shape: the stream of tools/history_trim_bench.py -- --old events over --users users with a Zipf(1.3) user distribution (one user owns about a quarter of
the events) -- with times uniform over 1000 values; per entry of --caps one cap.  The two results must agree: equal streams, equal row starts, equal
sorted segments (a sample of users).
usage: tools/history_cap_bench.py [--old N] [--users N] [--caps C,C] [--reps N] [--inner N] [--log FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from universal_recommender_amd import _lib  # noqa: E402
from universal_recommender_amd.device import DeviceSession  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--old", type=int, default=1 << 22)
ap.add_argument("--users", type=int, default=1 << 18)
ap.add_argument("--caps", default="64,500,5000", help="events a user keeps")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=20, help="calls per timed window; the printed times are per call")
ap.add_argument("--log", default=None, help="also write the lines to this file")
args = ap.parse_args()

assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
dev = torch.device("cuda", 0)
sess = DeviceSession(dev, _lib.load(os.environ.get("URCCO_LIB", _lib.DEFAULT_PATH)))
lines = []


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
    return f"{min(ms):.3f} ms best, {sorted(ms)[len(ms) // 2]:.3f} ms median of {len(ms)} ({[round(x, 3) for x in ms]})"


rng = np.random.default_rng(29)
n, n_users = args.old, args.users
h_users = ((rng.zipf(1.3, n) - 1) % n_users).astype(np.int32)
h_items = rng.integers(0, 1 << 20, n).astype(np.int32)
h_times = rng.integers(0, 1000, n).astype(np.int64)
users, items, times = (torch.from_numpy(a).to(dev) for a in (h_users, h_items, h_times))
rp, pos = sess.history_index(users, n_users)
sess.synchronize()
cnt = torch.diff(rp)
say(f"stream: {n} events over {n_users} users, Zipf(1.3): the largest user owns {int(cnt.max())} events, {int((cnt == 0).sum())} users own none; times uniform over 1000 values")
check = lambda status: _lib.check(status, sess.lib)  # noqa: E731
t_items, t_times, t_rp, t_pos = sess.empty(n, torch.int32), sess.empty(n, torch.int64), sess.empty(n_users + 1, torch.int64), sess.empty(n, torch.int32)
counts = sess.empty(2, torch.int64)
i_rp, i_pos = sess.empty(n_users + 1, torch.int64), sess.empty(n, torch.int32)
I64_MIN = -(1 << 63)


def host_filter(cap):
    """bool [n]: the events the cap keeps -- rank inside the user by (time, position) descending, below the cap"""
    order = np.lexsort((np.arange(n), h_times, h_users))            # by user, then time, then position, ascending
    start = np.concatenate([[0], np.cumsum(np.bincount(h_users, minlength=n_users))])
    from_end = start[h_users[order] + 1] - 1 - np.arange(n)       # 0 for a user's most recent event
    keep = np.zeros(n, bool)
    keep[order[from_end < cap]] = True
    return keep


def host_route(cap, out):
    t0 = time.perf_counter()
    keep = host_filter(cap)
    f = [a[keep] for a in (h_users, h_items, h_times)]
    t1 = time.perf_counter()
    d = [torch.from_numpy(a).to(dev) for a in f]
    check(sess.lib.urcco_dev_history_index(sess.handle, d[0].numel(), d[0].data_ptr(), n_users, i_rp.data_ptr(), i_pos.data_ptr()))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out["items"], out["times"] = d[1], d[2]
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


ms_floor = timed(lambda: check(sess.lib.urcco_dev_history_trim(sess.handle, n, items.data_ptr(), times.data_ptr(), n_users, rp.data_ptr(), pos.data_ptr(), I64_MIN, 0, None,
                                                               t_items.data_ptr(), t_times.data_ptr(), t_rp.data_ptr(), t_pos.data_ptr(), counts.data_ptr())), args.reps)
say(f"urcco_dev_history_trim, min_time_ms = INT64_MIN, nobody dropped (everything kept: the shared pipeline with the most to compact): {show(ms_floor)}")
for cap in [int(x) for x in args.caps.split(",")]:
    ms_c = timed(lambda: check(sess.lib.urcco_dev_history_cap(sess.handle, n, items.data_ptr(), times.data_ptr(), n_users, rp.data_ptr(), pos.data_ptr(), I64_MIN, 0, None, cap,
                                                             t_items.data_ptr(), t_times.data_ptr(), t_rp.data_ptr(), t_pos.data_ptr(), counts.data_ptr())), args.reps)
    k, ke = (int(x) for x in counts.cpu())
    other = {}
    host = [host_route(cap, other) for _ in range(max(args.reps // 2, 1))]
    assert k == ke == other["items"].numel(), "the two routes disagree on the number of kept events"
    assert torch.equal(t_items[:k], other["items"]) and torch.equal(t_times[:k], other["times"]), "the two streams differ"
    assert torch.equal(t_rp, i_rp), "the two indexes disagree on the row starts"
    h_rp = t_rp.cpu().numpy()
    for u in [0, 1, 2] + rng.integers(0, n_users, 200).tolist():
        assert torch.equal(torch.sort(t_pos[h_rp[u]:h_rp[u + 1]]).values, torch.sort(i_pos[h_rp[u]:h_rp[u + 1]]).values), f"user {u}: the segments differ"
    over = int((cnt > cap).sum())
    say(f"cap {cap}: {over} users above it ({int((cnt > max(cap, 64)).sum())} beyond a wave, {int((cnt > max(cap, 4096)).sum())} beyond the LDS class), {n - k} of {n} events dropped ({100.0 * (n - k) / n:.1f} %):")
    say(f"  urcco_dev_history_cap: {show(ms_c)}")
    say(f"  host route, {len(host)} run(s): numpy filter {min(h[0] for h in host):.1f} ms best, copies of {k} events + urcco_dev_history_index {min(h[1] for h in host):.1f} ms best "
        f"({[(round(a, 1), round(b, 1)) for a, b in host]})")
say(f"one run on one MI355X, HIP events around {args.inner} calls per window (times per call), two warm-up calls before the windows; the host route by wall-clock around "
    "device synchronisations; no alternation of the routes, no repeat on another box")
if args.log:
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
sess.close()
