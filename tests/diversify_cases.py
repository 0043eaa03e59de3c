"""The greedy MMR rule of decision D36 (include/urcco.h urcco_dev_diversify) as a plain numpy f64 loop -- the product, then the difference --
and the cases tests/test_sim_diversify.py and tests/test_gpu_diversify.py share.  Every comparison is exact: counts, ids, score bits (as int64), positions,
links at selection and the four statistics.  A problem: count [n], idx / score [n, width], sim (the matrix rows per item), penalty, num."""
import functools

import numpy as np
import torch

from eval_ref import bits, put
from explain_ref import csr
from universal_recommender_amd import _lib

N_ITEMS = 300
# (seed, rows, width, num, penalty): the lane-slot and bitmap-word edges; 400 and 3300 rows outnumber the grid's waves on the simulator and on the MI355X
CASES = [(1, 5, 1, 1, 0.25), (2, 9, 63, 63, 1.5), (3, 9, 63, 20, 0.0), (4, 9, 64, 64, 0.25), (5, 9, 64, 1, 1.5), (6, 9, 65, 65, 0.25), (7, 9, 65, 20, 1.5),
         (8, 9, 128, 128, 0.25), (9, 9, 128, 40, 0.0), (10, 9, 129, 129, 1.5), (11, 9, 129, 1, 0.25), (12, 9, 192, 192, 0.25), (13, 9, 192, 60, 1.5),
         (14, 9, 256, 256, 0.25), (15, 9, 256, 20, 1.5), (16, 9, 256, 1, 0.0), (17, 400, 128, 20, 0.25), (18, 3300, 3, 2, 1.5)]


def mmr(p, n_items=N_ITEMS):
    """The definition, row by row -> (count, idx, score bits, pos, links, [rows, matrix entries walked, linked pairs, rows left as their eligible prefix])"""
    n, width, num, sim = len(p["count"]), p["idx"].shape[1], p["num"], p["sim"]
    count, stats = np.zeros(n, np.int32), np.array([n, 0, 0, 0], np.int64)
    idx, pos, links, score = np.full((n, num), -1, np.int32), np.full((n, num), -1, np.int32), np.zeros((n, num), np.int32), np.zeros((n, num), np.int64)
    in_bits = bits(p["score"]).reshape(p["idx"].shape)
    for r in range(n):
        first, adj, alive, n_j = {}, np.zeros((width, width), bool), np.zeros(width, bool), np.zeros(width)
        for j in range(min(max(int(p["count"][r]), 0), width)):
            if 0 <= p["idx"][r, j] < n_items:
                first.setdefault(int(p["idx"][r, j]), j)
        for x, a in first.items():
            alive[a], stats[1] = True, stats[1] + len(sim[x])
            for y in sim[x]:
                if int(y) in first and int(y) != x:
                    adj[a, first[int(y)]] = adj[first[int(y)], a] = True
        elig, s = np.flatnonzero(alive), p["score"][r].astype(np.float64)
        top = s[elig].max() if len(elig) else 0.0
        w = np.float64(p["penalty"]) * top if top > 0 else np.float64(0.0)
        count[r] = min(num, len(elig))
        for t in range(count[r]):
            e = int(np.argmax(np.where(alive, s - w * n_j, -np.inf)))                           # product, then difference; the first of the largest keys
            idx[r, t], score[r, t], pos[r, t], links[r, t] = p["idx"][r, e], in_bits[r, e], e, n_j[e]
            alive[e], n_j = False, n_j + adj[e]
        stats[2:] += adj.sum() // 2, pos[r, : count[r]].tolist() == elig[: count[r]].tolist()
    return count, idx, score, pos, links, stats


def problem(seed, n, width, num, penalty):
    """Random rows over matrix rows of 0..6 entries in one direction, with self and out-of-catalogue entries and a hub (item 7: 3000 entries).  Row 0 is empty, row
    1 half filled; items repeat, two slots of a full row hold -1 and N_ITEMS.  Even rows score in eighths (keys tie), odd rows in random doubles (keys round)."""
    rng = np.random.default_rng(seed)
    sim = [np.concatenate([rng.permutation(N_ITEMS)[: rng.integers(0, 7)], [i, -3, N_ITEMS][: rng.integers(0, 4)]]).astype(np.int64) for i in range(N_ITEMS)]
    sim[7] = rng.integers(-2, N_ITEMS + 2, 3000)
    idx = rng.integers(0, N_ITEMS, (n, width)).astype(np.int32)
    if width > 2:
        idx[:, width // 3], idx[:, width // 2] = -1, N_ITEMS
    count = np.full(n, width, np.int32)
    count[:2] = (0, width // 2)
    score = np.where(np.arange(n)[:, None] % 2 == 0, rng.integers(0, 40, (n, width)) / 8.0, rng.random((n, width)))
    return dict(count=count, idx=idx, score=-np.sort(-score, axis=1), sim=sim, num=num, penalty=penalty)


def table(rows, scores, sim, num, penalty):
    return dict(count=np.array([len(r) for r in rows], np.int32), idx=np.array(rows, np.int32), score=np.array(scores, np.float64), sim=sim, num=num, penalty=penalty)


def constructed():
    """name -> problem: the matrices whose answer is known by eye"""
    none, ids, down = [np.zeros(0, np.int64)] * N_ITEMS, list(range(200)), list(np.arange(200, 0, -1.0))
    clique = [np.arange(200) if i < 200 else none[0] for i in range(N_ITEMS)]                     # every item names every item, itself included
    chain = [np.array([i + 1]) if i < 199 else none[0] for i in range(N_ITEMS)]                   # i -> i + 1 only: stored in one direction
    star = [np.random.default_rng(i).integers(-5, N_ITEMS + 5, 5000 if i == 0 else i % 3) for i in range(N_ITEMS)]
    return {"clique": table([ids, ids[::-1]], [down, down], clique, 200, 0.25), "chain": table([ids, ids[::2] + ids[1::2]], [down, down], chain, 200, 1.5),
            "star": table([ids, ids[100:] + ids[:100]], [down, down], star, 60, 0.25),
            # w = 0.25 x 4 = 1.  Step 0: keys 4, 4, 3, position 0.  Step 1: item 1 is linked to the chosen 0, 4 - 1 = 3 = the key of item 2: position 1
            "tie": table([[0, 1, 2]], [[4.0, 4.0, 3.0]], [np.array([1])] + none[1:], 3, 0.25),
            "zeros": table([ids[:70], ids[:70]], [[0.0] * 70, [0.0] * 35 + [-1.0] * 35], clique, 70, 1.5)}


def run(sess, p):
    """DeviceSession.diversify -> numpy (count, idx, score bits, pos, links, stats)"""
    n, width = p["idx"].shape
    rp, ci = (put(sess, a) for a in csr(p["sim"]))
    out = sess.diversify(put(sess, p["count"])[:n], put(sess, p["idx"])[: n * width].view(n, width), put(sess, p["score"])[: n * width].view(n, width), rp, ci,
                         p["penalty"], p["num"], N_ITEMS, stats=True)
    sess.synchronize()
    count, idx, score, pos, links = (t.cpu().numpy() for t in out[:5])
    return count, idx, bits(score).reshape(idx.shape), pos, links, out[5].cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(case):
    p = constructed()[case] if isinstance(case, str) else problem(*case)
    return p, mmr(p)


def check_case(sess, case):
    p, want = reference(case)
    got = run(sess, p)
    for name, g, w in zip(("count", "idx", "score", "pos", "links"), got, want):
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])
    assert got[5].tolist() == want[5].tolist() + [0] * 4, (got[5], want[5])
    return got


def check_constructed(sess):
    got = {name: check_case(sess, name) for name in constructed()}
    assert got["clique"][3][0, :3].tolist() == [0, 1, 2] and got["clique"][4][0, :3].tolist() == [0, 1, 2] and got["clique"][5][2] == 2 * (200 * 199 // 2)
    assert got["chain"][3][0, :4].tolist() == [0, 2, 4, 6] and got["chain"][5][2] == 2 * 199     # 1.5 x top: every other item first
    assert got["star"][5][1] > 2 * 5000                                                         # the hub's row is walked in both table rows
    assert got["tie"][3][0].tolist() == [0, 1, 2] and got["tie"][4][0].tolist() == [0, 1, 0]     # keys 4 - 1 = 3 and 3: the smaller position
    assert got["zeros"][3][0].tolist() == list(range(70)) and got["zeros"][5][3] == 2           # w = 0: the order is the input's


def check_arguments(sess):
    """no rows, the nullable outputs, and every URCCO_BAD_ARG case of include/urcco.h: the sizes, the penalty, each NULL the call needs"""
    p = problem(20, 4, 8, 3, 0.25)
    assert run(sess, dict(p, count=p["count"][:0], idx=p["idx"][:0], score=p["score"][:0]))[5].tolist() == [0] * 8
    keep = [put(sess, a) for a in (p["count"], p["idx"], p["score"]) + csr(p["sim"])] + [sess.empty(4, torch.int32), sess.empty(12, torch.int32), sess.empty(12, torch.float64)]
    c, i, s, rp, ci, oc, oi, os_ = (t.data_ptr() for t in keep)
    good = [sess.handle, 4, 8, c, i, s, N_ITEMS, rp, ci, 0.25, 3, oc, oi, os_, None, None, None]
    assert sess.lib.urcco_dev_diversify(*good) == _lib.OK                                       # out_pos, out_links and stats are nullable
    sess.synchronize()
    assert np.array_equal(keep[6].cpu().numpy().reshape(4, 3), mmr(p)[1])
    for d in [{0: None}, {1: -1}, {1: 1 << 31}, {2: 0}, {2: 257}, {10: 0}, {10: 9}, {9: -0.5}, {9: float("inf")}, {9: float("nan")}, {6: -1}, {3: None}, {4: None},
              {5: None}, {7: None}, {8: None}, {11: None}, {12: None}, {13: None}]:
        assert sess.lib.urcco_dev_diversify(*[d.get(at, a) for at, a in enumerate(good)]) == _lib.BAD_ARG, d
