"""Decision D35 (include/urcco.h urcco_dev_list_exposure / _exposure_stats / _list_links) in plain numpy and Python ints, and the cases the simulator
and GPU tests share.  Every integer is compared exactly; the floats of evaluate.list_metrics bit for bit with the host formulas over the reference integers."""
import os
from types import SimpleNamespace
from unittest import mock

import numpy as np
import torch

from eval_ref import bits, put, tree
from explain_ref import csr
from universal_recommender_amd import _lib
from universal_recommender_amd.evaluate import list_metrics

N_ITEMS = 300
# (seed, rows, num, ks, head): the rounds of 64 and their edges, one cut-off and eight, a cut-off equal to num and a last one below it, a grid that loops
CASES = [(1, 6, 1, (1,), False), (2, 9, 63, (63,), False), (3, 9, 64, (1, 2, 3, 5, 8, 13, 21, 64), True), (4, 9, 65, (10, 64), False),
         (5, 9, 256, (1, 5, 10, 20, 64, 65, 128, 256), True), (6, 400, 20, (1, 5, 10, 20), True), (7, 40, 256, (7, 200), False)]


def exposure_ref(p, n_items=N_ITEMS):
    bucket = np.zeros((len(p["ks"]), n_items), np.uint32)
    for q, c in enumerate(p["count"]):
        for j in range(min(min(max(int(c), 0), p["num"]), p["ks"][-1])):
            i = int(p["idx"][q, j])
            if 0 <= i < n_items:
                bucket[min(x for x, k in enumerate(p["ks"]) if j < k), i] += 1
    return bucket


def stats_ref(bucket):
    """(expo int64 [n_ks, n_items], [covered, total, sq, R] per cut-off as Python ints)"""
    expo = np.cumsum(bucket.astype(np.int64), axis=0)
    rows = [[int(v) for v in e] for e in expo]
    return expo, [[sum(v > 0 for v in e), sum(e), sum(v * v for v in e), sum((r + 1) * v for r, v in enumerate(sorted(e)))] for e in rows]


def links_ref(p, n_items=N_ITEMS):
    """(linked int32 [n, n_ks], sums int64 [2 n_ks])"""
    n, ks = len(p["count"]), p["ks"]
    linked, pairs = np.zeros((n, len(ks)), np.int32), np.zeros((n, len(ks)), np.int64)
    for q in range(n):
        c, first = min(max(int(p["count"][q]), 0), p["num"]), {}
        for j in range(c):
            i = int(p["idx"][q, j])
            if 0 <= i < n_items:
                first.setdefault(i, j)
        for x, k in enumerate(ks):
            m = min(k, c)
            linked[q, x], pairs[q, x] = sum(1 for ra, a in first.items() if a < m for rb in p["sim"][ra] if int(rb) != ra and first.get(int(rb), m) < m), m * (m - 1)
    return linked, np.concatenate([linked.sum(0, dtype=np.int64), pairs.sum(0)])


def floats_ref(p, stats, expo, linked, pop, n_items=N_ITEMS):
    """the host formulas of the decision over the reference integers"""
    ks, out = p["ks"], {"coverage": [], "gini": [], "herfindahl": [], "ils": [], "novelty": []}
    info = np.where(pop > 0, -np.log2(np.maximum(pop, 1).astype(np.float64) / np.float64(int(pop.sum()))), 0.0)
    for x, (covered, total, sq, big_r) in enumerate(stats):
        m = np.array([min(ks[x], min(max(int(c), 0), p["num"])) for c in p["count"]], np.int64)
        pairs = m * (m - 1)
        ratio = np.where(pairs > 0, linked[:, x].astype(np.float64) / np.maximum(pairs, 1).astype(np.float64), 0.0)
        terms = np.where((expo[x] > 0) & (pop > 0), expo[x].astype(np.float64) * info, 0.0)
        out["coverage"].append(covered / n_items)
        out["gini"].append(2 * big_r / (n_items * total) - (n_items + 1) / n_items if total else 0.0)
        out["herfindahl"].append(sq / total ** 2 if total else 0.0)
        out["ils"].append(float(tree(ratio)) / float((pairs > 0).sum()) if (pairs > 0).any() else 0.0)
        out["novelty"].append(float(tree(terms)) / float(total) if total else 0.0)
    return out


def problem(seed, n, num, ks, head):
    """Random rows; similarity rows of 0..6 entries, a self entry among them.  The first counts are 0, 1, num / 2, num, num + 7 and -3 (behind a count lie live
    items: a read there shows); two slots of every row hold -1 and N_ITEMS, one repeats its neighbour; head: item 7 leads every row."""
    rng = np.random.default_rng(seed)
    sim = [rng.permutation(N_ITEMS)[: rng.integers(0, 7)] for _ in range(N_ITEMS)]
    sim[11] = np.array([11, 12, 250])
    idx = rng.integers(0, N_ITEMS, (n, num)).astype(np.int32)
    if num > 4:
        idx[:, num // 3], idx[:, num // 2], idx[:, 3] = -1, N_ITEMS, idx[:, 2]
    if head:
        idx[:, 0] = 7
    count = np.full(n, num, np.int32)
    count[:6] = (0, 1, num // 2, num, num + 7, -3)
    return dict(count=count, idx=idx, num=num, ks=ks, sim=sim)


def planted(name):
    """"zero": every count is 0 or -3, nothing is shown (total == 0); "equal": every item of the catalogue exactly once inside the one cut-off"""
    p = problem(30, 15, 20, (20,), False)
    p["count"][:] = np.resize([0, -3], 15) if name == "zero" else 20
    return p if name == "zero" else dict(p, idx=np.arange(N_ITEMS, dtype=np.int32).reshape(15, 20))


def special():
    """a table row over similarity rows of 0, 1, 64, 65 and 300 entries (every item, itself included); 1 -> 5 without 5 -> 1; the second row runs backwards"""
    rng = np.random.default_rng(50)
    sim = [rng.permutation(N_ITEMS)[:n] for n in (0, 1, 64, 65, 300)] + [rng.permutation(N_ITEMS)[: rng.integers(0, 4)] for _ in range(N_ITEMS - 5)]
    sim[1], sim[5] = np.array([5]), np.array([9])
    row = np.concatenate([np.arange(5), 5 + rng.permutation(N_ITEMS - 5)[:251]]).astype(np.int32)
    return dict(count=np.array([256, 256], np.int32), idx=np.stack([row, row[::-1]]), num=256, ks=(1, 2, 5, 10, 64, 65, 200, 256), sim=sim)


def full():
    """every item names every item: the 256-wide row holds 256 * 255 linked pairs"""
    idx = np.stack([np.random.default_rng(s).permutation(N_ITEMS)[:256] for s in range(3)]).astype(np.int32)
    return dict(count=np.array([256, 256, 100], np.int32), idx=idx, num=256, ks=(128, 256), sim=[np.roll(np.arange(N_ITEMS), i) for i in range(N_ITEMS)])


def table(sess, p, lo=0, hi=None):
    n, num = p["idx"][lo:hi].shape
    return put(sess, p["count"][lo:hi])[:n], put(sess, p["idx"][lo:hi])[: n * num].view(n, num)


def run_exposure(sess, p, chunks=(None,), slots=None, n_items=N_ITEMS):
    """DeviceSession.list_exposure over the row ranges ending at `chunks`, into one bucket; slots: URCCO_EXPO_LDS_SLOTS for the calls"""
    with mock.patch.dict(os.environ, {"URCCO_EXPO_LDS_SLOTS": str(slots)} if slots else {}):
        bucket, lo = None, 0
        for hi in chunks:
            bucket, lo = sess.list_exposure(*table(sess, p, lo, hi), p["ks"], n_items, bucket), hi
        sess.synchronize()
    return bucket


def check_stats(sess, bucket):
    expo, stats = sess.exposure_stats(put(sess, bucket)[: bucket.size].view(bucket.shape))
    sess.synchronize()
    want_expo, want = stats_ref(bucket)
    assert np.array_equal(expo.cpu().numpy(), want_expo)
    assert [[int(v) % (1 << 64) for v in row] for row in stats.cpu().tolist()] == want, (stats, want)
    return want


def check_links(sess, p):
    rp, ci = (put(sess, a) for a in csr(p["sim"]))
    sums = torch.full((2 * len(p["ks"]),), 5, dtype=torch.int64, device=sess.device)                  # the sums are added to
    linked, sums = sess.list_links(*table(sess, p), rp, ci, p["ks"], N_ITEMS, sums)
    sess.synchronize()
    want, want_sums = links_ref(p)
    assert np.array_equal(linked.cpu().numpy(), want), np.argwhere(linked.cpu().numpy() != want)[:5]
    assert (sums.cpu().numpy() - 5).tolist() == want_sums.tolist()
    return want


def check_case(sess, case):
    """exposure (one call, three uneven chunks, a 16-slot table), statistics, links and the floats of list_metrics for one table: a random one of CASES, or a
    planted one whose exposure is all zero (every float 0.0) or equal (one tie block; gini the formula's rounding of 0)"""
    p = planted(case) if isinstance(case, str) else problem(*case)
    n, want = len(p["count"]), exposure_ref(p)
    for kw in (dict(), dict(chunks=(n // 5, n // 5 + 1, None)), dict(slots=16)):
        assert np.array_equal(run_exposure(sess, p, **kw).cpu().numpy(), want), kw
    stats, linked = check_stats(sess, want), check_links(sess, p)
    rp, ci = (put(sess, a) for a in csr(p["sim"]))
    model = SimpleNamespace(sess=sess, n_items=N_ITEMS, correlators=[SimpleNamespace(row_ptr=rp, col_idx=ci)])
    pop = np.random.default_rng(n).integers(0, 50, N_ITEMS) * (np.arange(N_ITEMS) % 7 > 0)
    got = list_metrics(model, *table(sess, p), p["ks"], popularity=pop, chunk=max(n // 3, 1))
    for key, w in floats_ref(p, stats, stats_ref(want)[0], linked, pop).items():
        assert np.array_equal(bits(np.array(got[key])), bits(np.array(w))), (key, got[key], w)
    assert got["covered"] == [s[0] for s in stats] and got["total"] == [s[1] for s in stats] and np.array_equal(got["bucket"].cpu().numpy(), want)
    assert np.array_equal(got["per_user"]["linked"].cpu().numpy(), linked) and "novelty" not in list_metrics(model, *table(sess, p), p["ks"])


BUCKETS = {"one item": np.eye(1, N_ITEMS, 17, dtype=np.uint32) * 4000, "single": np.array([[2], [0], [9]], np.uint32),
           "wide": np.random.default_rng(8).integers(0, 2 ** 20, (8, 5000)).astype(np.uint32)}


def check_arguments(sess):
    """no rows, no items, and the URCCO_BAD_ARG cases of include/urcco.h for the three calls"""
    p = problem(20, 8, 20, (1, 5, 10, 20), False)
    rp, ci = (put(sess, a) for a in csr(p["sim"]))
    count, idx = table(sess, p)
    assert not sess.list_exposure(count[:0], idx[:0], p["ks"], N_ITEMS).cpu().numpy().any() and sess.list_exposure(count, idx, p["ks"], 0).shape == (4, 0)
    assert sess.list_links(count[:0], idx[:0], rp, ci, p["ks"], N_ITEMS)[0].shape == (0, 4) and not sess.list_links(count, idx, rp, ci, p["ks"], 0)[0].cpu().numpy().any() \
        and sess.exposure_stats(torch.zeros((4, 0), dtype=torch.uint32, device=sess.device))[1].cpu().numpy().tolist() == [[0] * 4] * 4
    lib, h, N, k = sess.lib, sess.handle, N_ITEMS, lambda *v: (_lib.C.c_int32 * max(len(v), 1))(*v)
    keep = (count, idx, sess.empty(2 * N, torch.int32), sess.empty(2 * N, torch.int64), sess.empty(8, torch.int64))
    c, i, b, x, st = (t.data_ptr() for t in keep)
    good = [(lib.urcco_dev_list_exposure, (h, 8, 20, c, i, N, k(1), 1, b)), (lib.urcco_dev_exposure_stats, (h, N, 2, b, x, st)),
            (lib.urcco_dev_list_links, (h, 8, 20, c, i, N, rp.data_ptr(), ci.data_ptr(), k(1), 1, b, None))]
    # {argument: value}: a NULL the call needs, a negative size, num 0 and 257, n_rows * n_ks and n_ks * n_items at 2^31, no / nine / unordered / outlying cut-offs
    table_bad = [{0: None}, {1: -1}, {1: 1 << 31}, {2: 0}, {2: 257}, {3: None}, {4: None}, {5: -1}]
    ks_bad = lambda at: [{at: None}, {at + 1: 0}, {at: k(*range(1, 10)), at + 1: 9}, {at: k(5, 5), at + 1: 2}, {at: k(5, 1), at + 1: 2}, {at: k(0, 5), at + 1: 2}, {at: k(1, 21), at + 1: 2}]
    bad = [table_bad + ks_bad(6) + [{8: None}], [{0: None}, {1: -1}, {1: (1 << 31) - 1}, {2: 0}, {2: 9}, {3: None}, {4: None}, {5: None}],
           table_bad + ks_bad(8) + [{6: None}, {7: None}, {10: None}]]
    for (fn, args), cases in zip(good, bad):
        assert fn(*args) == _lib.OK
        for d in cases:
            assert fn(*[d.get(at, a) for at, a in enumerate(args)]) == _lib.BAD_ARG, (fn.__name__, d)
    sess.synchronize()
