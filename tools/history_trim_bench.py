#!/usr/bin/env python3
"""Times urcco_dev_history_trim (decision D22) against the other way to the same state -- a torch boolean-mask filter of the stream's `users`, `items`
and `times` arrays, then urcco_dev_history_index over the filtered `users` -- on the GPU: HIP events around windows of --inner calls, warm, several
repetitions; times are per call.  The outputs of the two library calls are allocated beforehand; the mask filter allocates its results through torch's
caching allocator and synchronises once per masked array (it has to learn the size), which is part of that route.

Shape: the old stream of tools/history_append_bench.py -- --old events over --users users with a Zipf(1.3) user distribution (one user owns about a
quarter of the events, about half of the users own none) -- with times uniform over 1000 values, and per entry of --drop a cut-off that drops about
that share of the events.  Printed per cut-off: both times, and the rate the byte count of the decision implies for the trim -- per stream position
its time (8 B), per kept event its item and time read again and written (24 B), per index entry its position read twice (8 B), per kept entry its
new position written (4 B), per user the row start read and written (16 B); bitmap, count and base traffic (about 1.5 B per position) and the gathers'
sector overhead are not in the count.  The two results must agree: equal streams, equal row starts, equal sorted segments (a sample of users).
--drop-heaviest: the user that owns the most events is dropped as well (one entry of drop_users; the other route masks `users != that id` too).
usage: tools/history_trim_bench.py [--old N] [--users N] [--drop PCT,PCT] [--drop-heaviest] [--reps N] [--inner N] [--log FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from universal_recommender_amd import _lib  # noqa: E402
from universal_recommender_amd.device import DeviceSession  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--old", type=int, default=1 << 22)
ap.add_argument("--users", type=int, default=1 << 18)
ap.add_argument("--drop", default="10,90", help="per cent of the events the cut-offs drop")
ap.add_argument("--drop-heaviest", action="store_true", help="also drop the user that owns the most events: the mark kernel's worst case, one listed user")
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
users = torch.from_numpy(((rng.zipf(1.3, n) - 1) % n_users).astype(np.int32)).to(dev)
items = torch.from_numpy(rng.integers(0, 1 << 20, n).astype(np.int32)).to(dev)
times = torch.from_numpy(rng.integers(0, 1000, n).astype(np.int64)).to(dev)
rp, pos = sess.history_index(users, n_users)
sess.synchronize()
cnt = torch.diff(rp)
say(f"stream: {n} events over {n_users} users, Zipf(1.3): the largest user owns {int(cnt.max())} events, {int((cnt == 0).sum())} users own none; times uniform over 1000 values")
check = lambda status: _lib.check(status, sess.lib)  # noqa: E731
t_items, t_times, t_rp, t_pos = sess.empty(n, torch.int32), sess.empty(n, torch.int64), sess.empty(n_users + 1, torch.int64), sess.empty(n, torch.int32)
counts = sess.empty(2, torch.int64)
i_rp, i_pos = sess.empty(n_users + 1, torch.int64), sess.empty(n, torch.int32)
other = {}
heavy = int(cnt.argmax())
drop = torch.tensor([heavy], dtype=torch.int32, device=dev) if args.drop_heaviest else None
n_drop, drop_ptr = (1, drop.data_ptr()) if drop is not None else (0, None)


def other_route(cut):
    mask = times >= cut
    if drop is not None:
        mask &= users != heavy
    u, other["items"], other["times"] = users[mask], items[mask], times[mask]
    check(sess.lib.urcco_dev_history_index(sess.handle, u.numel(), u.data_ptr(), n_users, i_rp.data_ptr(), i_pos.data_ptr()))


for pct in [int(x) for x in args.drop.split(",")]:
    cut = pct * 10
    ms_t = timed(lambda: check(sess.lib.urcco_dev_history_trim(sess.handle, n, items.data_ptr(), times.data_ptr(), n_users, rp.data_ptr(), pos.data_ptr(), cut, n_drop, drop_ptr,
                                                             t_items.data_ptr(), t_times.data_ptr(), t_rp.data_ptr(), t_pos.data_ptr(), counts.data_ptr())), args.reps)
    ms_o = timed(lambda: other_route(cut), args.reps)
    k, ke = (int(x) for x in counts.cpu())
    assert k == ke == other["items"].numel(), "the two routes disagree on the number of kept events"
    assert torch.equal(t_items[:k], other["items"]) and torch.equal(t_times[:k], other["times"]), "the two streams differ"
    assert torch.equal(t_rp, i_rp), "the two indexes disagree on the row starts"
    h_rp = t_rp.cpu().numpy()
    for u in [0, 1, 2] + rng.integers(0, n_users, 200).tolist():
        assert torch.equal(torch.sort(t_pos[h_rp[u]:h_rp[u + 1]]).values, torch.sort(i_pos[h_rp[u]:h_rp[u + 1]]).values), f"user {u}: the segments differ"
    n_bytes = 8 * n + 24 * k + 8 * n + 4 * ke + 16 * n_users
    say(f"cut-off {'and one dropped user of ' + str(int(cnt[heavy])) + ' events ' if drop is not None else ''}that drop{'' if drop is not None else 's'} {n - k} of {n} events ({100.0 * (n - k) / n:.1f} %):")
    say(f"  urcco_dev_history_trim: {show(ms_t)}")
    say(f"  torch mask filter of users / items / times + urcco_dev_history_index over the filtered users ({k} events): {show(ms_o)}")
    say(f"  bytes of the trim by the decision's count: 8 x {n} + 24 x {k} + 8 x {n} + 4 x {ke} + 16 x {n_users} = {n_bytes}; over the best time of the whole call: "
        f"{n_bytes / (min(ms_t) * 1e-3) / 1e9:.1f} GB/s")
say(f"one run on one MI355X, HIP events around {args.inner} calls per window (times per call), two warm-up calls before the windows; no alternation of the two routes, no repeat on another box; "
    + ("one listed user: the mark kernel runs, HT_SPLIT blocks share its chunks" if drop is not None else "no users dropped (n_drop = 0: the mark kernel does not run)"))
if args.log:
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
sess.close()
