#!/usr/bin/env python3
"""Times urcco_dev_dictionary_extend (decision D26) on the GPU: one batch of --batch events of Zipf(--zipf)-distributed users, --new per cent of them events
of users never seen, into a table of --ids ids -- against
  1. urcco_dev_dictionary_lookup of the same batch: the floor the old-key path should sit near (it answers -1 for the new users and changes nothing);
  2. urcco_dev_dictionary_build over every key seen so far, the batch included: the only device route to the same table before this call existed.
Every repetition uses a batch of its own (an extend changes the table: its new users are old the next time) and runs the three routes one after the other,
lookup first; wall-clock around device synchronisations (the extend and the build synchronise themselves), best and median of --reps.  The first extend
of the run is printed apart: the table, built over --ids keys, has the capacity of exactly those and is rehashed once by the capacity rule.
Checked per repetition: the ids of the batch's old users equal the lookup's, the number of new ids is the number of distinct new users, and the rebuilt
table has as many ids as the extended one.
usage: tools/dictionary_extend_bench.py [--ids N] [--batch N] [--new PCT] [--zipf A] [--reps N] [--log FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from universal_recommender_amd import _lib, ingest  # noqa: E402
from universal_recommender_amd.device import DeviceSession  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ids", type=int, default=1 << 24)
ap.add_argument("--batch", type=int, default=1 << 20)
ap.add_argument("--new", type=float, default=1.0, help="per cent of a batch's events that belong to users never seen")
ap.add_argument("--zipf", type=float, default=1.2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--log", default=None, help="also write the lines to this file")
args = ap.parse_args()

assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
dev = torch.device("cuda", 0)
sess = DeviceSession(dev, _lib.load(os.environ.get("URCCO_LIB", _lib.DEFAULT_PATH)))
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def show(ms):
    return f"{min(ms):.3f} ms best, {sorted(ms)[len(ms) // 2]:.3f} ms median of {len(ms)} ({[round(x, 3) for x in ms]})"


MULT = np.uint64(0x9E3779B97F4A7C15)      # odd: user number -> key is one to one, and spreads over the 64 bits
rng = np.random.default_rng(26)
n_ids, n = args.ids, args.batch
key_of = lambda numbers: (numbers.astype(np.uint64) + np.uint64(1)) * MULT      # noqa: E731
base = torch.from_numpy(key_of(rng.permutation(n_ids)).view(np.int64)).to(dev)
ms_build0, d = wall(lambda: ingest.dictionary_build(sess, base))
assert d.n_ids == n_ids
say(f"table: urcco_dev_dictionary_build over {n_ids} distinct keys, {ms_build0:.1f} ms (one run, cold)")


def batch(rep):
    """Zipf over the old users; about --new per cent of the positions hold users of this batch alone, each once or a few times"""
    who = (rng.zipf(args.zipf, n) - 1) % n_ids
    fresh = rng.random(n) < args.new / 100.0
    n_fresh = int(fresh.sum())
    who[fresh] = n_ids + rep * n + rng.integers(0, max(n_fresh * 3 // 4, 1), n_fresh)      # a quarter of them repeat inside the batch
    return torch.from_numpy(key_of(who).view(np.int64)).to(dev), fresh, int(np.unique(who[fresh]).size)


seen = [base]
ms_l, ms_e, ms_b = [], [], []
for rep in range(args.reps + 1):      # repetition 0 carries the rehash and the cold caches: printed apart
    keys, fresh, n_new = batch(rep)
    t_l, ids_l = wall(lambda: ingest.dictionary_lookup(sess, d, keys))
    before = d.n_ids
    t_e, (ids_e, new_pos) = wall(lambda: d.extend(keys))
    seen.append(keys)
    everything = torch.cat(seen)
    t_b, one = wall(lambda: ingest.dictionary_build(sess, everything))
    old = torch.from_numpy(~fresh).to(dev)
    assert torch.equal(ids_e[old], ids_l[old]) and bool((ids_l[~old] == -1).all()), "extend and lookup disagree on the old users"
    assert d.n_ids - before == n_new == int(new_pos.numel()) and one.n_ids == d.n_ids, "the routes disagree on the number of ids"
    assert torch.equal(ingest.dictionary_lookup(sess, one, keys), ids_e), "the rebuilt table answers otherwise"
    n_all = int(everything.numel())
    one.close()
    del everything
    if rep == 0:
        say(f"first batch ({n} events, {n_new} new users; the table grows from 2 x {n_ids} slots by one rehash): lookup {t_l:.3f} ms, extend {t_e:.3f} ms, "
            f"build over all {n_all} keys {t_b:.1f} ms")
    else:
        ms_l.append(t_l); ms_e.append(t_e); ms_b.append(t_b)
say(f"batches of {n} events, Zipf({args.zipf}) over the {n_ids} old users, {args.new} % of the events from new users; the table holds {d.n_ids} ids at the end")
say(f"  urcco_dev_dictionary_lookup (the floor; no new ids): {show(ms_l)}")
say(f"  urcco_dev_dictionary_extend (ids + new_pos, synchronises): {show(ms_e)}")
say(f"  urcco_dev_dictionary_build over every key seen so far (the route before): {show(ms_b)}")
say(f"one run on one MI355X, wall-clock around device synchronisations, one call per figure; the three routes alternate batch by batch (lookup, extend, build); the lookup "
    f"allocates its output through torch, as the extend does for ids and new_pos; nothing was repeated on another box")
if args.log:
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
d.close()
sess.close()
