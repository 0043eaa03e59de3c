#!/usr/bin/env python3
"""Times urcco_dev_history_append (decision D21) against the other way to the same index, urcco_dev_history_index over the concatenated `users`
array, on the GPU: HIP events around windows of --inner calls, warm, several repetitions, outputs allocated beforehand; times are per call.

Shape: an old stream of --old events over --users users with a Zipf(1.3) user distribution (one user owns about a quarter of the events, about half
of the users own none), and per entry of --batches a batch of that many events of the same distribution.  Printed per batch: both times, and the rate
the byte count of the decision implies for the append -- 8 B per old index entry (4 read, 4 written) plus 12 B per new event (its user read by the
count and by the scatter, its position written), over the time of the whole call; the row starts (24 B per user) are listed apart.  The two indexes
must agree: equal row starts, equal sorted segments (checked on a sample of users).
usage: tools/history_append_bench.py [--old N] [--users N] [--batches N,N] [--reps N] [--inner N] [--log FILE]"""
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
ap.add_argument("--batches", default="4096,409600")
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
n_old, n_users = args.old, args.users
old_users = torch.from_numpy(((rng.zipf(1.3, n_old) - 1) % n_users).astype(np.int32)).to(dev)
old_rp, old_pos = sess.history_index(old_users, n_users)
sess.synchronize()
cnt = torch.diff(old_rp)
say(f"old stream: {n_old} events over {n_users} users, Zipf(1.3): the largest user owns {int(cnt.max())} events, {int((cnt == 0).sum())} users own none")
check = lambda status: _lib.check(status, sess.lib)  # noqa: E731
for n_new in [int(x) for x in args.batches.split(",")]:
    new_users = torch.from_numpy(((rng.zipf(1.3, n_new) - 1) % n_users).astype(np.int32)).to(dev)
    all_users = torch.cat([old_users, new_users])
    a_rp, a_pos = sess.empty(n_users + 1, torch.int64), sess.empty(n_old + n_new, torch.int32)
    i_rp, i_pos = sess.empty(n_users + 1, torch.int64), sess.empty(n_old + n_new, torch.int32)
    ms_a = timed(lambda: check(sess.lib.urcco_dev_history_append(sess.handle, n_old, n_users, old_rp.data_ptr(), old_pos.data_ptr(), n_new, new_users.data_ptr(),
                                                               n_users, a_rp.data_ptr(), a_pos.data_ptr())), args.reps)
    ms_i = timed(lambda: check(sess.lib.urcco_dev_history_index(sess.handle, n_old + n_new, all_users.data_ptr(), n_users, i_rp.data_ptr(), i_pos.data_ptr())), args.reps)
    assert torch.equal(a_rp, i_rp), "the two indexes disagree on the row starts"
    h_rp = a_rp.cpu().numpy()
    for u in [0, 1, 2] + rng.integers(0, n_users, 200).tolist():
        assert torch.equal(torch.sort(a_pos[h_rp[u]:h_rp[u + 1]]).values, torch.sort(i_pos[h_rp[u]:h_rp[u + 1]]).values), f"user {u}: the segments differ"
    n_bytes = 8 * n_old + 12 * n_new
    say(f"batch of {n_new} events behind {n_old}:")
    say(f"  urcco_dev_history_append: {show(ms_a)}")
    say(f"  urcco_dev_history_index over the concatenated users array ({n_old + n_new} events): {show(ms_i)}")
    say(f"  bytes of the append by the decision's count: 8 x {n_old} + 12 x {n_new} = {n_bytes} (row starts apart: 24 x {n_users} = {24 * n_users}); over the best time of the "
        f"whole call: {n_bytes / (min(ms_a) * 1e-3) / 1e9:.1f} GB/s")
say(f"one run on one MI355X, HIP events around {args.inner} calls per window (times per call), two warm-up calls before the windows; no alternation of the two calls, no repeat on another box")
if args.log:
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
sess.close()
