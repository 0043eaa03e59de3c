"""The quota rule of decision D34 (include/urcco.h urcco_dev_quota_cut) as the plain sequential walk in Python, and the cases
tests/test_sim_quota.py and tests/test_gpu_quota.py share.  Every comparison is exact: counts, ids, score bits (as int64), `short`, and the statistics
the host can predict -- tier split, examined, rejected, short rows.  A problem: count [n], idx / score [n, width], rules of (rows per item, max), num."""
import os

import numpy as np
import pytest

from eval_ref import bits, put
from explain_ref import csr
from universal_recommender_amd import _lib

N_ITEMS = 300
# (seed, rows, width, num, the rules' maxima): the cut inside a round and on its edge, one / two / four rules, several hundred rows
CASES = [(1, 5, 1, 1, (1,)), (2, 9, 63, 63, (2,)), (3, 9, 63, 20, (1,)), (4, 9, 64, 64, (1,)), (5, 9, 64, 20, (2,)), (6, 9, 64, 1, (1,)), (7, 9, 65, 65, (2,)),
         (8, 9, 65, 20, (1, 2)), (9, 9, 256, 256, (1,)), (10, 9, 256, 20, (2, 1, 3, 1)), (11, 9, 256, 1, (2,)), (12, 400, 128, 20, (2,)), (13, 300, 200, 20, (1, 3))]


def walk(p):
    """The definition, row by row -> (count, idx, score bits, short, [lds rows, global rows, examined, rejected, short rows]) for a wave table of
    p["slots"] slots: a row leaves the LDS tier when the rounds of 64 it walks hold more values, repeats included, than 3/4 of the slots."""
    n, width, num = len(p["count"]), p["idx"].shape[1], p["num"]
    count, short = np.zeros(n, np.int32), np.zeros(n, np.int32)
    idx, score, stats = np.full((n, num), -1, np.int32), np.zeros((n, num), np.int64), np.zeros(5, np.int64)
    in_bits = bits(p["score"]).reshape(p["idx"].shape)
    for r in range(n):
        held, seen, m = {}, 0, min(max(int(p["count"][r]), 0), width)
        for j in range(m):
            if count[r] == num:
                break
            item, seen = int(p["idx"][r, j]), j + 1
            keys = [(q, int(v)) for q, (rows, _) in enumerate(p["rules"]) for v in rows[item]] if 0 <= item < N_ITEMS else None
            if keys is None or any(held.get(k, 0) >= p["rules"][k[0]][1] for k in keys):
                stats[3] += 1
                continue
            for k in keys:
                held[k] = held.get(k, 0) + 1
            idx[r, count[r]], score[r, count[r]] = item, in_bits[r, j]
            count[r] += 1
        short[r] = count[r] < num and m == width
        walked = p["idx"][r, : -(-seen // 64) * 64][: m]
        values = sum(len(rows[i]) for i in walked if 0 <= i < N_ITEMS for rows, _ in p["rules"])
        stats[1 if values > p["slots"] // 4 * 3 else 0] += 1
        stats[2] += seen
    stats[4] = short.sum()
    return count, idx, score, short, stats


def problem(seed, n, width, num, maxima):
    """Random rows over a catalogue whose items hold 0, 1 or 3 of twelve values per rule.  Row 0 is empty, row 1 half filled, the others full (a short
    row with a part-filled and with a full pool); items repeat, and two slots of every full row hold -1 and N_ITEMS."""
    rng = np.random.default_rng(seed)
    rules = [([np.sort(rng.permutation(12)[: rng.choice([0, 1, 3])]) for _ in range(N_ITEMS)], m) for m in maxima]
    idx = rng.integers(0, N_ITEMS, (n, width)).astype(np.int32)
    if width > 2:
        idx[:, width // 3], idx[:, width // 2] = -1, N_ITEMS
    count = np.full(n, width, np.int32)
    count[:2] = (0, width // 2)
    return dict(count=count, idx=idx, score=-np.sort(-rng.random((n, width)), axis=1), rules=rules, num=num)


def one_value(most):
    """64 candidates of one value in one round: exactly `most` are kept, the first ones"""
    return dict(count=np.array([64], np.int32), idx=np.arange(64, dtype=np.int32)[None, :], score=np.arange(64, 0, -1.0)[None, :],
                rules=[([np.zeros(1, np.int64)] * N_ITEMS, most)], num=64)


def chain():
    """Items {0, 1}, {1, 2}, {2, 3}, ... under max = 1: candidate l is kept iff l - 1 was rejected -- every fate hangs on the one before it"""
    return dict(count=np.array([65, 65], np.int32), idx=np.tile(np.arange(65, dtype=np.int32), (2, 1)), score=np.tile(np.arange(65, 0, -1.0), (2, 1)),
                rules=[([np.array([i, i + 1]) for i in range(N_ITEMS)], 1)], num=65)


def run(sess, p, slots=None):
    """DeviceSession.quota_cut -> numpy (count, idx, score bits, short, stats); slots: URCCO_QUOTA_LDS_SLOTS for the call"""
    n, width = p["idx"].shape
    rules = [tuple(put(sess, a) for a in csr(rows)) + (m,) for rows, m in p["rules"]]
    if slots is not None:
        os.environ["URCCO_QUOTA_LDS_SLOTS"] = str(slots)
    try:
        out = sess.quota_cut(put(sess, p["count"])[:n], put(sess, p["idx"])[: n * width].view(n, width), put(sess, p["score"])[: n * width].view(n, width),
                             rules, p["num"], N_ITEMS)
        sess.synchronize()
    finally:
        os.environ.pop("URCCO_QUOTA_LDS_SLOTS", None)
    count, idx, score, short, stats = (t.cpu().numpy() for t in out)
    return count, idx, bits(score).reshape(idx.shape), short, stats


def check(sess, p, slots=None):
    got, want = run(sess, p, slots), walk(dict(p, slots=slots or _lib.QUOTA_LDS_SLOTS))
    for name, g, w in zip(("count", "idx", "score", "short"), got, want):
        assert np.array_equal(g, w), name
    stats = got[4]
    assert stats[[0, 1, 2, 3, 5]].tolist() == want[4].tolist() and not stats[6:].any(), (stats, want[4])
    return got, want[4]


def check_case(sess, case, slots):
    _, tiers = check(sess, problem(*case), slots)
    assert slots is None or case[2] < 63 or tiers[1] > 0                                          # a lowered table sends full rows to the global tier


def check_rounds(sess, slots):
    for most in (1, 2):
        assert check(sess, one_value(most), slots)[0][0][0] == most
    got, _ = check(sess, chain(), slots)
    assert got[1][0, :33].tolist() == list(range(0, 65, 2)) and got[4][4] > 2 * 2                 # resolve iterations beyond the rows' two rounds each


def check_arguments(sess):
    """no rows, and every URCCO_BAD_ARG case of include/urcco.h: the sizes, the rules, a candidate with 193 values (its row and slot are named)"""
    p = problem(20, 4, 8, 3, (1,))
    assert run(sess, dict(p, count=p["count"][:0], idx=p["idx"][:0], score=p["score"][:0]))[0].size == 0
    wide = dict(p, idx=np.zeros((4, 257), np.int32), score=np.zeros((4, 257)))
    for q in [dict(p, num=0), dict(p, num=9), wide, dict(p, rules=[]), dict(p, rules=p["rules"] * 5), dict(p, rules=[(p["rules"][0][0], 0)])]:
        with pytest.raises(_lib.UrccoError) as e:
            run(sess, q)
        assert e.value.status == _lib.BAD_ARG
    rows = [np.arange(193 if i == 7 else 192 if i == 8 else 1) for i in range(N_ITEMS)]
    idx = np.full((4, 8), 8, np.int32)
    check(sess, dict(p, idx=idx, rules=[(rows, 1)]))                                             # 192 values: served
    idx[2, 5] = 7
    with pytest.raises(_lib.UrccoError, match="row 2, slot 5") as e:
        run(sess, dict(p, idx=idx, rules=[(rows, 1)]))
    assert e.value.status == _lib.BAD_ARG
