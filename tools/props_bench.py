#!/usr/bin/env python3
"""Times the device-resident item properties (decision D25) next to the route that exists without them, on the GPU, on the same aggregated map:
  host route     recommend._device_properties(dict): the Python loop over the aggregated dict that builds the item x value matrices and the date arrays
                 inside DeviceModel.from_indicators(properties=...).  After an inventory change it is the only route: the whole dict again
  device route   DeviceProperties.apply_streams (the dense-id tensor form: the events as they would arrive from the device ingest) + materialise, for
                 the first load and then for an update of --update of the items; and DeviceProperties.from_property_map (the dict form, split per key
                 in Python) + materialise for the first load
Shape: --items items, two list properties ("categories" over 1000 values, "tags" over 50 000) of 1-4 values each, three dates; the update sets every
property of a tenth of the items again.  Wall-clock times around a device synchronisation (the host work is part of both routes), --reps repetitions of
the device calls; the host route runs once per phase (it takes seconds).  The matrices of from_property_map must equal the host route's bit for bit.
No ratio is claimed: the lines say what one run on one box gave.
usage: tools/props_bench.py [--items N] [--update F] [--reps N] [--log FILE]"""
import argparse
import os
import sys
import time
from datetime import datetime, timezone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from universal_recommender_amd import _lib  # noqa: E402
from universal_recommender_amd.device import DeviceSession  # noqa: E402
from universal_recommender_amd.properties import DeviceProperties  # noqa: E402
from universal_recommender_amd.recommend import _device_properties  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=1 << 20)
ap.add_argument("--update", type=float, default=0.1, help="fraction of the items the update sets again")
ap.add_argument("--reps", type=int, default=5)
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

    def item_index(self, item):
        return int(item) if 0 <= int(item) < self.n_items else None


def draw(rng, items):
    """per list property (val_ptr, value ids), per date int64 milliseconds, for the given items"""
    out = {}
    for name, n_cols in LISTS.items():
        vp = np.zeros(items.size + 1, np.int64)
        np.cumsum(rng.integers(1, 5, items.size), out=vp[1:])
        out[name] = (vp, rng.integers(0, n_cols, int(vp[-1])).astype(np.int32))
    for name in DATES:
        out[name] = (T0 + 1000 * rng.integers(-10**6, 10**6, items.size)).astype(np.int64)
    return out


def as_dict(items, drawn, into=None):
    """the aggregated map in the form from_indicators(properties=...) takes: value strings, ISO dates"""
    into = {} if into is None else into
    iso = {name: [datetime.fromtimestamp(ms / 1000.0, tz=timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ") for ms in drawn[name].tolist()] for name in DATES}
    for k, i in enumerate(items.tolist()):
        f = into.setdefault(i, {})
        for name in LISTS:
            vp, vals = drawn[name]
            f[name] = [f"v{v}" for v in vals[vp[k]:vp[k + 1]].tolist()]
        for name in DATES:
            f[name] = iso[name][k]
    return into


def streams_of(items, drawn, t):
    times = np.full(items.size, t, np.int64)
    return {name: (items, times, None, drawn[name]) for name in list(LISTS) + DATES}


rng = np.random.default_rng(45)
n = args.items
model = Model(n)
all_items = np.arange(n, dtype=np.int32)
first = draw(rng, all_items)
upd_items = np.sort(rng.choice(n, int(n * args.update), replace=False)).astype(np.int32)
second = draw(rng, upd_items)
say(f"{n} items, list properties {LISTS} of 1-4 values, dates {DATES}; the update sets all five properties of {upd_items.size} items again")
names = {name: [f"v{j}" for j in range(c)] for name, c in LISTS.items()}

# ---- device route, tensor form -----------------------------------------------------------------------------------------------------------------------
load_ms, mat_ms, upd_ms, mat2_ms = [], [], [], []
for _ in range(args.reps):
    dp = DeviceProperties(sess, model, DATES)
    dp.apply_streams({}, new_values=names)
    load_ms.append(wall(lambda: dp.apply_streams(streams_of(all_items, first, 0)))[0])
    mat_ms.append(wall(dp.materialise)[0])
    upd_ms.append(wall(lambda: dp.apply_streams(streams_of(upd_items, second, 10)))[0])
    ms, (props_dev, dates_dev) = wall(dp.materialise)
    mat2_ms.append(ms)
mask_ms = [wall(dp.item_mask)[0] for _ in range(args.reps)]
say(f"device route, first load: apply_streams of 5 x {n} events (host numpy arrays -> device -> state) {show(load_ms)}")
say(f"    materialise (2 x bounds + rows + column counts + transposition, 3 x dates) {show(mat_ms)}")
say(f"device route, update: apply_streams of 5 x {upd_items.size} events {show(upd_ms)}")
say(f"    materialise {show(mat2_ms)}")
say(f"    item_mask {show(mask_ms)}")

# ---- host route, and the dict form of the device route --------------------------------------------------------------------------------------------
ms_dict, properties = wall(lambda: as_dict(all_items, first))
say(f"building the aggregated dict itself (not part of either route): {ms_dict:.0f} ms")
ms_host, (props_host, dates_host) = wall(lambda: _device_properties(sess, properties, DATES, n, model.item_index))
say(f"host route, first load: _device_properties(dict) {ms_host:.0f} ms (one run)")
ms_map, dp_map = wall(lambda: DeviceProperties.from_property_map(sess, model, properties, DATES))
ms_mat, (props_map, dates_map) = wall(dp_map.materialise)
say(f"device route, dict form: from_property_map(dict) {ms_map:.0f} ms + materialise {ms_mat:.2f} ms (one run)")
def by_column(p):
    """the CSC's entries as sorted (column, row) keys: urcco_dev_transpose leaves the order inside a column unspecified"""
    col = torch.repeat_interleave(torch.arange(p.n_cols, device=dev), p.col_ptr[1:] - p.col_ptr[:-1])
    return torch.sort(col * n + p.row_idx[: col.numel()].long()).values


for name, a in props_host.items():
    b = props_map[name]
    assert a.values == b.values and all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("row_ptr", "col_idx", "col_ptr")) and torch.equal(by_column(a), by_column(b)), name
assert all(torch.equal(dates_host[k], dates_map[k]) for k in DATES)
as_dict(upd_items, second, properties)
ms_host2, (props_host2, dates_host2) = wall(lambda: _device_properties(sess, properties, DATES, n, model.item_index))
say(f"host route, after the update: _device_properties(the whole dict again) {ms_host2:.0f} ms (one run)")
for name, a in props_host2.items():       # the tensor form numbers its values itself: the rows hold the same number of values, the dates are equal
    assert torch.equal(a.row_ptr, props_dev[name].row_ptr), name
assert all(torch.equal(dates_host2[k], dates_dev[k]) for k in DATES)
say("the dict form's CSR, column starts and dates equal the host route's bit for bit, its CSC rows column by column; the tensor form's rows have the host route's "
    "lengths and its dates are equal")
say(f"one run on one MI355X, wall-clock around device synchronisations; the host route's time includes its Python loop over the dict and {3 * n} date parses, the "
    "device route's apply_streams includes the host-to-device copies of the event arrays; nothing was alternated or repeated on another box")
if args.log:
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
sess.close()
