"""Plain numpy / Python restatement of decision D30 (include/urcco.h urcco_dev_explain) and the checks tests/test_sim_explain.py and
tests/test_gpu_explain.py share.  M_c = the sum of the clamped weights over set(T_c(q)) ^ row i of I_c, the listed terms = Python's sorted() on
(-contrib, clause, term) cut to max_terms, the score fold in Python floats.  Every comparison is exact: integers equal, doubles as bits.
A problem is (n_items, num, count, idx, clauses, max_terms) with clauses of (n_cols, boost, m_row_ptr, m_col_idx, q_row_ptr, q_col_idx, weight | None)."""
import os

import numpy as np

from eval_ref import bits, put
from universal_recommender_amd import _lib
from universal_recommender_amd.device import DevCsr

ONE, WMAX, SENTINEL = _lib.REC_WEIGHT_ONE, _lib.REC_WEIGHT_MAX, -7
CASES = [("edges", 1), ("edges", 5), ("edges", 64), ("order", 1), ("order", 2), ("order", 16), ("staging",), ("slots", 1), ("slots", 4), ("slots", 5), ("slots", 256)]


def csr(rows):
    rp = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    return rp, np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(1, np.int64)]).astype(np.int32)


def restate(n_items, num, count, idx, clauses, max_terms):
    """-> m [nq, num, n_clauses], n [nq, num], {(q, j): [(contrib, clause, term), ...]}"""
    m, n, terms = np.zeros((len(count), num, len(clauses)), np.int64), np.zeros((len(count), num), np.int32), {}
    for q in range(len(count)):
        for j in range(min(max(int(count[q]), 0), num)):
            i, found = int(idx[q, j]), []
            for c, (n_cols, boost, rp, ci, qrp, qci, w) in enumerate(clauses if 0 <= i < n_items else ()):
                for h in set(qci[qrp[q]:qrp[q + 1]].tolist()) & {h for h in ci[rp[i]:rp[i + 1]].tolist() if 0 <= h < n_cols}:
                    wt = ONE if w is None else min(max(int(w[h]), 1), WMAX)
                    m[q, j, c] += wt
                    found.append((-(boost * (float(wt) * 2.0 ** -15)), c, h))
            terms[q, j] = [(-x, c, h) for x, c, h in sorted(found)[:max_terms]]
            n[q, j] = len(terms[q, j])
    return m, n, terms


def call(sess, n_items, num, count, idx, clauses, max_terms):
    """urcco_dev_explain through ctypes over outputs filled with SENTINEL -> (status, m, n, clause, term, contrib) in numpy"""
    nq, nc = len(count), len(clauses)
    arr = (_lib.ExplainClause * nc)()
    keep = [put(sess, np.asarray(count, np.int32)), put(sess, np.asarray(idx, np.int32))]
    for c, (n_cols, boost, *arrays) in enumerate(clauses):
        keep += [None if a is None else put(sess, np.asarray(a, np.uint32) if k == 4 else a) for k, a in enumerate(arrays)]
        arr[c].n_cols, arr[c].boost = n_cols, boost
        arr[c].m_row_ptr, arr[c].m_col_idx, arr[c].q_row_ptr, arr[c].q_col_idx, arr[c].weight = (None if t is None else t.data_ptr() for t in keep[-5:])
    shape = ((nc, np.int64), (1, np.int32), (max_terms, np.int32), (max_terms, np.int32), (max_terms, np.float64))
    outs = [put(sess, np.full(nq * num * k, SENTINEL, dt)) for k, dt in shape]
    st = sess.lib.urcco_dev_explain(sess.handle, nq, n_items, num, keep[0].data_ptr(), keep[1].data_ptr(), arr, nc, max_terms, *[t.data_ptr() for t in outs])
    sess.synchronize()
    return (st,) + tuple(t[: nq * num * k].cpu().numpy().reshape(nq, num, k) for t, (k, _) in zip(outs, shape))


def check(sess, n_items, num, count, idx, clauses, max_terms):
    """two runs equal each other and the restatement; the sentinel survives wherever the contract writes nothing"""
    idx = np.asarray(idx, np.int32).reshape(len(count), num)
    got, again = (call(sess, n_items, num, count, idx, clauses, max_terms) for _ in range(2))
    assert got[0] == _lib.OK and all(a.tobytes() == b.tobytes() for a, b in zip(got[1:], again[1:]))
    m, n, terms = restate(n_items, num, count, idx, clauses, max_terms)
    assert np.array_equal(got[1], m) and np.array_equal(got[2][:, :, 0], n)
    for q, j in np.ndindex(len(count), num):
        k, want = int(n[q, j]), terms.get((q, j), [])
        assert [(int(bits(x)[0]), c, h) for x, c, h in want] == [(int(bits(got[5][q, j, r])[0]), int(got[3][q, j, r]), int(got[4][q, j, r])) for r in range(k)], (q, j)
        assert all((g[q, j, k:] == SENTINEL).all() for g in got[3:]), (q, j)


# ---- the smallest shapes at which the kernel can go wrong ---------------------------------------------------------------------------------------------
def edges(max_terms):
    """rounds of 64 and the buffer of 128: row lengths 0 .. 300 against a query row of every column (matches = row length); a weighted second clause, empty
    for query 0 (the totals stay exact) and full for query 1 (prunes across clauses); half rows for query 2"""
    rng = np.random.default_rng(max_terms)
    lens = sorted({0, 1, 63, 64, 65, 127, 128, 129, 300, max_terms - 1, max_terms, max_terms + 1})
    i0, i1 = csr([rng.permutation(300)[:n] for n in lens]), csr([rng.permutation(300)[: rng.integers(0, 90)] for _ in lens])
    half = np.sort(rng.permutation(300)[:150])
    t0, t1 = csr([np.arange(300), np.arange(300), half]), csr([[], np.arange(300), half])
    return len(lens), len(lens), [len(lens)] * 3, np.tile(np.arange(len(lens)), 3), [(300, 1.0) + i0 + t0 + (None,), (300, 0.75) + i1 + t1 + (rng.integers(1, 4 * ONE, 300),)], max_terms


def order(n_clauses):
    """search edges and the total order: matches at the first and the last term, an empty term row, row entries outside 0..n_cols, an all-empty clause, ties
    inside an unweighted clause, 2.0 * 1.0 == 1.0 * 2.0 across clauses 0 and 2, weights 0, 1, ONE, MAX and MAX + 1 under the clamp"""
    rng = np.random.default_rng(n_clauses)
    rows = [[20, -1, 3, 40, 2 ** 31 - 1], [10], list(rng.permutation(40)), [], [0, 39, 5, 4, 3, 2, 1], [40, -5]]
    t, w = csr([[3, 10, 20], np.arange(40), [], [0, 39]]), rng.integers(1, 3 * ONE, 40)
    w[:6] = [0, 1, ONE, WMAX, WMAX + 1, 2 * ONE]
    clauses = [(40, 2.0) + csr(rows) + t + (None,), (40, 1.5) + csr(rows[::-1]) + csr([[]] * 4) + (None,), (40, 1.0) + csr(rows) + t + (w,)]
    clauses += [(40, c / 64) + csr([rng.permutation(40)[: rng.integers(0, 30)] for _ in rows]) + t + (None,) for c in range(3, 16)]
    return 6, 6, [6] * 4, np.tile(np.arange(6), 4), clauses[:n_clauses], 16


def staging():
    """one batch on both sides of EXPLAIN_LDS_TERMS: L(q) = 8192 in one clause and split, 8193 in one clause and split"""
    rng = np.random.default_rng(4)
    rows = [np.concatenate([[0, 4095, 4096, 8191, 8192], rng.permutation(8000)[:100] + 100]) for _ in range(4)]
    t0, t1 = csr([np.arange(8192), np.arange(8193), np.arange(4097), np.arange(4096)]), csr([[], [], np.arange(4097, 8193), np.arange(4096, 8192)])
    assert _lib.EXPLAIN_LDS_TERMS == 8192
    return 4, 4, [4] * 4, np.tile(np.arange(4), 4), [(8193, 1.0) + csr(rows) + t0 + (None,), (8193, 0.5) + csr(rows[::-1]) + t1 + (rng.integers(1, 4 * ONE, 8193),)], 64


def slots(num):
    """every count around num, clamped ones, ids -1 and n_items inside the count, poison behind it"""
    rng = np.random.default_rng(num)
    count, idx = [0, 1, num - 1, num, -3, num + 7], rng.integers(0, 300, (6, num))
    idx[3, 0], idx[5, num - 1] = -1, 300
    for q, c in enumerate(count):
        idx[q, min(max(c, 0), num):] = 10 ** 9
    t = csr([np.sort(rng.permutation(50)[: rng.integers(0, 50)]) for _ in count])
    return 300, num, count, idx, [(50, b) + csr([rng.permutation(50)[: rng.integers(0, 12)] for _ in range(300)]) + t + (None,) for b in (1.0, 3.0)], 5


def check_score(sess, weighted, limit=256):
    """urcco_dev_recommend_weighted, then explain over the same clauses: the fold of out_m is out_score bit for bit in both classes of the recommend kernels"""
    rng = np.random.default_rng(6)
    n_items, nq, num, rec, expl = 300, 40, 20, [], []
    for n_cols, boost in ((300, 1.0), (80, 0.3)):
        rp, ci = csr([rng.permutation(n_cols)[: rng.integers(0, 20)] for _ in range(n_items)])
        # every fourth query is light (the LDS class): no term at all (pure backfill) or one term of the first clause (a few scores, then backfill)
        t = csr([np.sort(rng.permutation(n_cols)[: rng.integers(0, 60) if q % 4 else int(q % 8 == 4 and n_cols == 300)]) for q in range(nq)])
        d = [put(sess, a) for a in (rp, ci) + t]
        cp, ri = sess.transpose(DevCsr(n_items, n_cols, d[0], d[1], int(rp[-1])), sess.column_counts(d[1], int(rp[-1]), n_cols))
        rec.append((n_cols, boost, cp, ri, d[2], d[3]))
        expl.append((n_cols, boost) + tuple(d) + (sess.idf_weights(cp, n_cols, n_items) if weighted else None,))
    os.environ["URCCO_REC_LDS_LIMIT"] = str(limit)
    try:
        count, idx, score, stats = sess.recommend(nq, n_items, rec, num, weights=[c[6] for c in expl])
    finally:
        del os.environ["URCCO_REC_LDS_LIMIT"]
    m, n = sess.explain(count, idx, expl, 5, n_items)[:2]
    sess.synchronize()
    count, score, stats, m, n = (x.cpu().numpy() for x in (count, score, stats, m, n))
    folded = np.zeros((nq, num))
    for q, j in np.ndindex(nq, num):
        for c, boost in enumerate((1.0, 0.3)):
            folded[q, j] = folded[q, j] + boost * (float(int(m[q, j, c])) * 2.0 ** -15)
    assert stats[0] > 0 and stats[1] > 0 and (count == num).all() and (score > 0).any() and (score == 0.0).any()
    assert np.array_equal(bits(folded), bits(score)) and ((n == 0) == (score == 0.0)).all()


def check_arguments(sess):
    """n_queries == 0 and every URCCO_BAD_ARG case of include/urcco.h"""
    n_items, num, count, idx, clauses, e = order(2)
    run = lambda n_items=n_items, num=num, count=count, clauses=clauses, e=e: call(sess, n_items, num, count, np.zeros(len(count) * max(num, 1)), clauses, e)[0]
    assert run() == _lib.OK and run(count=[]) == _lib.OK and run(e=64) == _lib.OK and run(num=256) == _lib.OK
    for bad in (dict(num=0), dict(num=257), dict(e=0), dict(e=65), dict(n_items=-1), dict(clauses=clauses[:1] * 17), dict(clauses=[(-1,) + clauses[0][1:]]),
                *(dict(clauses=[(40, b) + clauses[0][2:]]) for b in (0.0, -1.0, float("inf"), float("nan")))):
        assert run(**bad) == _lib.BAD_ARG, bad
    arr = (_lib.ExplainClause * 1)()
    zeros = put(sess, np.zeros(64, np.int64))                                                    # every array of a one-query call with an empty table
    p = zeros.data_ptr()
    arr[0].n_cols, arr[0].boost, arr[0].m_row_ptr, arr[0].m_col_idx, arr[0].q_row_ptr, arr[0].q_col_idx = 4, 1.0, p, p, p, p
    full = [sess.handle, 1, 4, 1, p, p, arr, 1, 1, p, p, p, p, p]
    assert sess.lib.urcco_dev_explain(*full) == _lib.OK
    for k in (0, 4, 5, 6, 9, 10, 11, 12, 13):                                                    # the session, the table, the clauses, an output
        assert sess.lib.urcco_dev_explain(*[None if x == k else v for x, v in enumerate(full)]) == _lib.BAD_ARG, k
    for name in ("m_row_ptr", "m_col_idx", "q_row_ptr", "q_col_idx"):                            # a NULL matrix array of a clause
        setattr(arr[0], name, None)
        assert sess.lib.urcco_dev_explain(*full) == _lib.BAD_ARG, name
        setattr(arr[0], name, p)
    assert sess.lib.urcco_dev_explain(*full[:1] + [(1 << 31) // 64] + full[2:8] + [64] + full[9:]) == _lib.BAD_ARG   # n_queries * num * max_terms = 2^31
    assert sess.lib.urcco_dev_explain(*full[:1] + [-1] + full[2:]) == _lib.BAD_ARG
    sess.synchronize()
