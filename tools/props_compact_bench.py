#!/usr/bin/env python3
"""Times DeviceProperties.compact (decision D28) on the GPU: a store that took the first load of --items items and then --rounds updates of a tenth of
the items each -- every stream holds (1 + rounds / 10) x items events, of which one per item still wins -- is compacted:
  materialise over the uncompacted store, compact (every property; one read of the counts), materialise over the compacted store
Shape: tools/props_bench.py's -- two list properties ("categories" over 1000 values, "tags" over 50 000) of 1-4 values each, three dates.  Wall-clock
around device synchronisations, --reps repetitions, each on a store built afresh (a compacted store has nothing left to compact).  The store must
answer after the compaction as before: matrices, dates and mask bit for bit.  No ratio is claimed: the lines say what one run on one box gave.
usage: tools/props_compact_bench.py [--items N] [--rounds N] [--reps N] [--log FILE]"""
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
from universal_recommender_amd.properties import DeviceProperties  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=1 << 20)
ap.add_argument("--rounds", type=int, default=20, help="updates of a tenth of the items each, after the first load")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--log", default=None, help="also write the lines to this file")
args = ap.parse_args()

assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
dev = torch.device("cuda", 0)
sess = DeviceSession(dev, _lib.load(os.environ.get("URCCO_LIB", _lib.DEFAULT_PATH)))
lines = []
LISTS = {"categories": 1000, "tags": 50_000}
DATES = ["date", "available", "expires"]
T0 = 1_700_000_000_000


def say(line):
    print(line, flush=True)
    lines.append(line)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def show(ms):
    return f"{min(ms):.2f} ms best, {sorted(ms)[len(ms) // 2]:.2f} ms median of {len(ms)} ({[round(x, 2) for x in ms]})"


class Model:
    def __init__(self, n_items):
        self.sess, self.n_items = sess, n_items


def draw(rng, items, t):
    out = {}
    times = np.full(items.size, t, np.int64)
    for name, n_cols in LISTS.items():
        vp = np.zeros(items.size + 1, np.int64)
        np.cumsum(rng.integers(1, 5, items.size), out=vp[1:])
        out[name] = (items, times, None, (vp, rng.integers(0, n_cols, int(vp[-1])).astype(np.int32)))
    for name in DATES:
        out[name] = (items, times, None, (T0 + 1000 * rng.integers(-10**6, 10**6, items.size)).astype(np.int64))
    return out


def build():
    rng = np.random.default_rng(45)
    dp = DeviceProperties(sess, Model(n), DATES)
    dp.apply_streams({}, new_values={name: [f"v{j}" for j in range(c)] for name, c in LISTS.items()})
    dp.apply_streams(draw(rng, np.arange(n, dtype=np.int32), 0))
    for r in range(args.rounds):
        dp.apply_streams(draw(rng, np.sort(rng.choice(n, n // 10, replace=False)).astype(np.int32), 10 + r))
    return dp


def shot(dp):
    props, dates = dp.materialise()
    return [getattr(p, f) for p in props.values() for f in ("row_ptr", "col_idx", "col_ptr")] + list(dates.values()) + [dp.item_mask()]


n = args.items
say(f"{n} items, list properties {LISTS} of 1-4 values, dates {DATES}; the first load and {args.rounds} updates of {n // 10} items each")
mat_before, compact_ms, mat_after = [], [], []
for _ in range(args.reps):
    dp = build()
    before = shot(dp)
    mat_before.append(wall(dp.materialise)[0])
    sizes = {name: (s.n_events, s.n_values) for name, s in dp.streams.items()}
    compact_ms.append(wall(dp.compact)[0])
    mat_after.append(wall(dp.materialise)[0])
    assert all(torch.equal(a, b) for a, b in zip(before, shot(dp))), "the compacted store answers differently"
say("per property (events before -> after, values before -> after): " + ", ".join(f"{name} {e0} -> {e1}, {v0} -> {v1}" for name, (e0, e1, v0, v1) in dp.last_compact.items()))
say(f"materialise over the uncompacted store: {show(mat_before)}")
say(f"compact (5 calls, one read of the counts, the gathers of items / times / kinds): {show(compact_ms)}")
say(f"materialise over the compacted store: {show(mat_after)}")
say("matrices, dates and mask after the compaction equal those before, bit for bit")
say("one run on one MI355X, wall-clock around device synchronisations, every repetition on a store built afresh; nothing was alternated or repeated on another box")
if args.log:
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
sess.close()
