"""Numpy restatement of decision D33 (include/urcco.h urcco_dev_audience) and the cases tests/test_sim_audience.py and
tests/test_gpu_audience.py share.  Per clause an exact integer count M (units of 2^-15) from dense 0/1 matrices, the f64 fold in clause order, the
exclusions, np.lexsort on (-score, user id) cut to num.  Every comparison is exact: counts and ids equal, scores as bits.
A problem: items (query positions -> catalogue items), clauses of (n_cols, boost, item rows, user rows, weight | None), excl rows, uids, num."""
import os

import numpy as np
import pytest

from eval_ref import bits, put
from explain_ref import csr
from universal_recommender_amd import _lib

ONE, WMAX, N_ITEMS, N_COLS, BOOSTS = _lib.REC_WEIGHT_ONE, _lib.REC_WEIGHT_MAX, 150, (80, 30, 50), (1.05, 20.0, 0.3)
# (seed, users, query items, num): the wave and round edges, the tile edges, "E+d": num = the hub item's audience + d
CASES = [(1, 1, 5, 7), (2, 63, 5, 7), (3, 64, 1, 7), (4, 65, 5, 7), (5, 257, 5, 3), (6, 600, 5, 1), (7, 600, 64, 9), (8, 300, 65, 9), (9, 300, 130, 9),
         (10, 90, 5, "E-1"), (11, 90, 5, "E+0"), (12, 90, 5, "E+1")]


def dense(rows, n_cols):
    d = np.zeros((len(rows), n_cols), np.int64)
    for r, row in enumerate(rows):
        d[r, [h for h in row if 0 <= h < n_cols]] = 1
    return d


def scores(p):
    s = np.zeros((len(p["uids"]), len(p["items"])))
    for n_cols, boost, irows, urows, w in p["clauses"]:
        wt = np.full(n_cols, ONE, np.int64) if w is None else np.clip(np.asarray(w, np.int64), 1, WMAX)
        m = (dense(urows, n_cols) * wt) @ dense([irows[i] for i in p["items"]], n_cols).T
        s = s + boost * (m.astype(np.float64) * 2.0 ** -15)                                 # (double)(m * 2^15) * 2^-15 == (double)m: one fold for both forms
    return s


def reference(p):
    """-> per query position (user ids, scores) in the order (score desc, user id asc), cut to num"""
    s, uids, out = scores(p), p["uids"], []
    for x, item in enumerate(p["items"]):
        us = np.flatnonzero((s[:, x] > 0) & (uids >= 0) & ~np.array([item in e for e in p["excl"]], bool))
        order = us[np.lexsort((uids[us], -s[us, x]))][: p["num"]]
        out.append((uids[order], s[order, x]))
    return out


def problem(seed, n_users, n_query, num, weighted=False):
    """Random rows under the boosts of recommend_ref.  Users 0 .. 3 hold 0, 1, 64, 65 terms in clause 0.  Item 0 holds the hub alone -- column 0 of clause 0,
    which three users in four share: one score for all of them, the user id decides every cut, and from 260 users on its list passes the compaction
    mark.  Item 1 has empty rows; item 2 is queried twice; query position 4's best user excludes that item; the last user's id is -1 (nobody)."""
    rng = np.random.default_rng(seed)
    irows = [[rng.permutation(n)[: rng.integers(0, 8)] for _ in range(N_ITEMS)] for n in N_COLS]
    urows = [[np.sort(1 + rng.permutation(n - 1)[: rng.integers(0, 10)]) for _ in range(n_users)] for n in N_COLS]
    for c in range(3):
        irows[c][0], irows[c][1] = np.arange(int(c == 0)), np.arange(0)
    for u, n in enumerate((0, 1, 64, 65)[:n_users]):
        urows[0][u] = np.sort(1 + rng.permutation(N_COLS[0] - 1)[: max(n - 1, 0)])              # (users 1 .. 3 get the hub below)
    urows[0] = [np.union1d(r, [0]) if u % 4 else r for u, r in enumerate(urows[0])]
    uids = rng.permutation(2 * n_users + 8)[:n_users].astype(np.int32)
    if n_users > 8:
        uids[-1] = -1
    w = [rng.choice([1, ONE, WMAX], n) if weighted and c != 1 else None for c, n in enumerate(N_COLS)]
    p = dict(items=np.array(([0, 1, 2, 2] + list(range(3, N_ITEMS)))[:n_query], np.int32), uids=uids, num=1,
             clauses=[(n, b, ir, ur, wc) for n, b, ir, ur, wc in zip(N_COLS, BOOSTS, irows, urows, w)],
             excl=[np.sort(3 + rng.permutation(N_ITEMS - 3)[: rng.integers(0, 5)]) for _ in range(n_users)])
    if n_query > 4 and len(reference(p)[4][0]):
        u = int(np.flatnonzero(uids == reference(p)[4][0][0])[0])
        p["excl"][u] = np.union1d(p["excl"][u], [p["items"][4]])
    p["num"] = num if isinstance(num, int) else max(1, int((scores(p)[:, 0] > 0)[uids >= 0].sum()) + int(num[1:]))
    return p


def run(sess, p, chunks=(1.0,), items=None, num=None):
    """DeviceSession.audience over the users cut at the given fractions, accumulating -> (count, user, score, stats summed) in numpy"""
    n_users, out, stats = len(p["uids"]), None, np.zeros(_lib.AUD_STATS_LEN, np.int64)
    items = p["items"] if items is None else np.asarray(items, np.int32)
    d_items = put(sess, items)[: len(items)]
    imats = [tuple(put(sess, a) for a in csr(ir)) for _, _, ir, _, _ in p["clauses"]]
    cuts = [0] + [int(round(f * n_users)) for f in np.cumsum(chunks)]
    for lo, hi in zip(cuts, cuts[1:]):
        clauses = [(n, b) + im + tuple(put(sess, a) for a in csr(ur[lo:hi])) + (None if w is None else put(sess, np.asarray(w, np.uint32)),)
                   for (n, b, _, ur, w), im in zip(p["clauses"], imats)]
        excl = tuple(put(sess, a) for a in csr(p["excl"][lo:hi]))
        *out, st = sess.audience(d_items, N_ITEMS, clauses, p["num"] if num is None else num, hi - lo, put(sess, p["uids"][lo:hi]), excl, out)
        sess.synchronize()
        stats += st.cpu().numpy()
    return tuple(t.cpu().numpy() for t in out) + (stats,)


def check(sess, p, **how):
    count, user, score, stats = run(sess, p, **how)
    for x, (us, sc) in enumerate(reference(p)):
        k = len(us)
        assert count[x] == k and np.array_equal(user[x, :k], us) and np.array_equal(bits(score[x, :k]), bits(sc)), x
        assert (user[x, k:] == -1).all() and (score[x, k:] == 0.0).all(), x
    assert stats[4] == 0                                                                      # no table or list overflow, ever
    return count, user, score, stats


def check_case(sess, case, weighted=False):
    p = problem(*case, weighted=weighted)
    stats = check(sess, p)[3]
    n_hub = len(reference(dict(p, num=1 << 30))[0][0])                                         # a list longer than num + 256 at a round's end is cut
    assert stats[0] == -(-len(p["items"]) // 64) and stats[1] == 1 and (stats[2] > 0 or n_hub <= p["num"] + 256), (stats, n_hub)


def check_chunks(sess):
    """one chunk and three unequal chunks give the bits of the reference, so each other's; 4 500 users, some 3 400 of them on the hub, at num = 1024: two
    slabs, each cut on the way"""
    p = problem(21, 700, 6, 5)
    a, b = check(sess, p), check(sess, p, chunks=(0.13, 0.5, 0.37))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3][2] > 0 and b[3][1] == 3
    stats = check(sess, problem(13, 4500, 4, 1024))[3]
    assert stats[1] == 2 and stats[2] >= 2


def check_tiles(sess):
    """URCCO_AUD_TERMS = the pairs of the largest item: twelve items fall into at least three tiles; one pair less, and that item fails the call"""
    p = problem(22, 200, 12, 6)
    pairs = [sum(len(ir[i]) for _, _, ir, _, _ in p["clauses"]) for i in p["items"]]
    os.environ["URCCO_AUD_TERMS"] = str(max(pairs))
    try:
        assert check(sess, p)[3][0] >= 3
        os.environ["URCCO_AUD_TERMS"] = str(max(pairs) - 1)
        with pytest.raises(_lib.UrccoError, match=rf"items\[{int(np.argmax(pairs))}\]") as e:
            run(sess, p)
        assert e.value.status == _lib.BAD_ARG
    finally:
        del os.environ["URCCO_AUD_TERMS"]


def check_arguments(sess):
    """no users, no items, and every URCCO_BAD_ARG case of include/urcco.h that the binding can state"""
    p = problem(23, 20, 5, 4)
    assert run(sess, p, items=[])[0].size == 0 and not run(sess, dict(p, uids=p["uids"][:0], excl=[], clauses=[c[:3] + ([],) + c[4:] for c in p["clauses"]]))[0].any()
    bad_boost = [dict(p, clauses=[p["clauses"][0][:1] + (b,) + p["clauses"][0][2:]]) for b in (0.0, -1.0, float("inf"), float("nan"))]
    for q, how in [(p, dict(num=0)), (p, dict(num=1025)), (p, dict(items=[0, N_ITEMS])), (p, dict(items=[-1])), (dict(p, clauses=[]), {}),
                   (dict(p, clauses=p["clauses"][:1] * 17), {}), (dict(p, clauses=[(-1,) + p["clauses"][0][1:]]), {})] + [(q, {}) for q in bad_boost]:
        with pytest.raises(_lib.UrccoError) as e:
            run(sess, q, **how)
        assert e.value.status == _lib.BAD_ARG, how
