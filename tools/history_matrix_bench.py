#!/usr/bin/env python3
"""Times urcco_dev_history_users + urcco_dev_history_matrix (decision D23) against the other way to the same matrix -- urcco_dev_csr_from_pairs over the
same events with the `users` array that a history no longer has -- on the GPU: HIP events around windows of --inner calls, warm, several repetitions;
times are per call.  All outputs are allocated beforehand.  The pairs route gets its row numbers (row_of[users]) precomputed outside the timed window
and is called without its nnz read-back, so neither route synchronises.

Shape: the stream of tools/history_append_bench.py -- --events events over --users users with a Zipf(1.3) user distribution (one user owns about a
quarter of the events, about half of the users own none), items uniform over --cols columns, no times (the open window), min_events 1.  Timed twice:
the whole stream, whose heaviest user is the bitmap class's one-row worst case, and the stream without that user's events.  Printed per stream: both
times, the users per class, and the byte count of the decision's cost model for the two calls -- per index entry its position read twice and its item
once (12 B), per user two row starts, row_of, the row's length and start written and read (48 B), per matrix entry the raw row written and read and
the result written (12 B), per heavy row one atomic exchange per bitmap word (4 B); the bit sets, the scans and the gathers' sector overhead are not in
the count.  The two results must agree: row_ptr and col_idx[:nnz] bit for bit.
usage: tools/history_matrix_bench.py [--events N] [--users N] [--cols N] [--reps N] [--inner N] [--log FILE]"""
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
ap.add_argument("--events", type=int, default=1 << 22)
ap.add_argument("--users", type=int, default=1 << 18)
ap.add_argument("--cols", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=10, help="calls per timed window; the printed times are per call")
ap.add_argument("--log", default=None, help="also write the lines to this file")
args = ap.parse_args()

assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
dev = torch.device("cuda", 0)
sess = DeviceSession(dev, _lib.load(os.environ.get("URCCO_LIB", _lib.DEFAULT_PATH)))
lines = []
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


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


check = lambda status: _lib.check(status, sess.lib)  # noqa: E731
rng = np.random.default_rng(29)
n_users, n_cols = args.users, args.cols
all_users = ((rng.zipf(1.3, args.events) - 1) % n_users).astype(np.int32)
all_items = rng.integers(0, n_cols, args.events).astype(np.int32)
heavy = int(np.bincount(all_users, minlength=n_users).argmax())
say(f"stream: {args.events} events over {n_users} users, Zipf(1.3), items uniform over {n_cols} columns, no times, min_events 1")

for name, sel in (("the whole stream", np.ones(args.events, bool)), ("without the heaviest user's events", all_users != heavy)):
    users, items = torch.from_numpy(all_users[sel]).to(dev), torch.from_numpy(all_items[sel]).to(dev)
    n = int(users.numel())
    rp, pos = sess.history_index(users, n_users)
    sess.synchronize()
    cnt = torch.diff(rp)
    row_of, n_rows_dev = sess.empty(n_users, torch.int32), sess.empty(1, torch.int64)
    users_call = lambda: check(sess.lib.urcco_dev_history_users(sess.handle, n, None, n_users, rp.data_ptr(), pos.data_ptr(), I64_MIN, I64_MAX, 1,  # noqa: E731
                                                                row_of.data_ptr(), n_rows_dev.data_ptr()))
    users_call()
    n_rows = int(n_rows_dev.item())
    m_rp, m_ci, m_nnz = sess.empty(n_rows + 1, torch.int64), sess.empty(n, torch.int32), sess.empty(1, torch.int64)
    p_rp, p_ci = sess.empty(n_rows + 1, torch.int64), sess.empty(n, torch.int32)
    rows = row_of[users.long()].contiguous()      # the pairs route's row numbers: outside the timed window
    matrix_call = lambda: check(sess.lib.urcco_dev_history_matrix(sess.handle, n, items.data_ptr(), None, n_users, rp.data_ptr(), pos.data_ptr(), I64_MIN, I64_MAX,  # noqa: E731
                                                                  n_cols, row_of.data_ptr(), n_rows, m_rp.data_ptr(), m_ci.data_ptr(), n, m_nnz.data_ptr()))

    def history_route():
        users_call()
        matrix_call()

    pairs_route = lambda: check(sess.lib.urcco_dev_csr_from_pairs(sess.handle, n, rows.data_ptr(), items.data_ptr(), n_rows, p_rp.data_ptr(), p_ci.data_ptr(), None))  # noqa: E731
    ms_h, ms_u, ms_m, ms_p = timed(history_route, args.reps), timed(users_call, args.reps), timed(matrix_call, args.reps), timed(pairs_route, args.reps)
    nnz = int(m_nnz.item())
    assert torch.equal(m_rp, p_rp) and torch.equal(m_ci[:nnz], p_ci[:nnz]), "the two routes disagree"
    wave, block, bitmap = int(((cnt > 0) & (cnt <= 64)).sum()), int(((cnt > 64) & (cnt <= 4096)).sum()), int((cnt > 4096).sum())
    words = (n_cols + 31) // 32
    n_bytes = 12 * n + 48 * n_users + 12 * nnz + 4 * words * bitmap
    say(f"{name}: {n} events, the largest user owns {int(cnt.max())}, {int((cnt == 0).sum())} users own none; rows by class: {wave} wave, {block} block, {bitmap} bitmap "
        f"({words} words per bitmap); {n_rows} rows, {nnz} entries")
    say(f"  urcco_dev_history_users + urcco_dev_history_matrix: {show(ms_h)}")
    say(f"    urcco_dev_history_users alone: {show(ms_u)}")
    say(f"    urcco_dev_history_matrix alone: {show(ms_m)}")
    say(f"  urcco_dev_csr_from_pairs over (row_of[users], items), the row numbers precomputed: {show(ms_p)}")
    say(f"  bytes of the two calls by the decision's count: 12 x {n} + 48 x {n_users} + 12 x {nnz} + 4 x {words} x {bitmap} = {n_bytes}; over the best time of the two calls: "
        f"{n_bytes / (min(ms_h) * 1e-3) / 1e9:.1f} GB/s")
say(f"one run on one MI355X, HIP events around {args.inner} calls per window (times per call), two warm-up calls before the windows; no alternation of the routes, no repeat on "
    "another box; the inputs of every call are those of the call before and stay in the caches")
if args.log:
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
sess.close()
