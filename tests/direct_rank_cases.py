"""Workloads and a plain-numpy model of the direct ranking of the packed row kernels (csrc/cco_rows.hip, direct_limit), shared by test_sim_direct_rank.py and
test_gpu_direct_rank.py: a row of a class that carries the k11 = 1 prefilter whose C valid candidates number more than k and at most the class's limit is
ranked at once, without a select.  Every case compares the build with the same build under NO_DIRECT_RANK bit for bit and with the oracle; COUNT_DIRECT
(stats[30] while stage timing is on) reports the rows that were ranked directly."""
import numpy as np

from helpers import check_indicators, compare_with_oracle, run_device, sort_rows, to_dev, to_params
from oracle import c_oracle as O
from prefilter_cases import CLAMP_BIN, assert_bit_equal, crafted
from universal_recommender_amd import _lib

N_BIG = 200_000             # users: cA cB << N for every candidate of the crafted rows
# the accumulator classes that carry the prefilter (bin numbers of cco_kernels.h) -- direct_limit(T, E) of cco_rows.hip, 0 = compiled out of the class --
# and the capacity of their ambiguous-set arrays (what the edges are taken around where a class has no direct ranking)
DIRECT_LIMIT = {1: 0, 2: 128, 3: 128, 4: 128, 5: 128}
SEL_M = {1: 64, 2: 128, 3: 128, 4: 128, 5: 128}
TABLE_WORDS = {1: 1024, 2: 4096, 3: 8192, 4: 16384, 5: 32768}
CLASS_SIZES = {1: (100, 280), 2: (300, 1200), 3: (1500, 2600), 4: (3000, 5000), 5: (6000, 10000)}   # distinct candidates of the crafted rows (k = 50, cA = 4)


def class_of(w, ca, n_cols, k):
    """choose_bin of cco_rows.hip for rows whose counts fit the packed field."""
    if w <= 64 and ca <= 64:
        return 0
    dmax = 3 * min(w, n_cols) + 3 * k + 2
    cap = next((c for c in (1, 2, 3, 4, 5) if dmax <= TABLE_WORDS[c]), 6)
    return max(cap, 1 if w <= 512 else (2 if w <= 8192 else 4))


def survivor_counts(k, above=80, multi=5, plain=3):
    """cb_of for `crafted`: a row of D candidates whose first s = survivors - multi k11 = 1 columns get the counts 1 .. k - 1 and then k, again and again --
    k of them at or below c* = k exactly when s >= k, all s of them when the tie at c* is kept whole -- and the rest a count above c* and inside the
    limit, which the prefilter drops.  `survivors` per row, in the order `crafted` draws the rows."""
    def make(survivors):
        it = iter(survivors)

        def cb_of(rng, n):
            s = next(it) - multi
            assert k <= s <= n - multi, (s, n)
            cb = np.full(n, above, np.int64)
            cb[:multi] = plain                                        # the k11 = 2 columns
            cb[multi:multi + s] = np.minimum(np.arange(1, s + 1), k)  # distinct small counts, then the tie at the cut
            return cb
        return cb_of
    return make


def general(sizes, ca, n_users, k11_of, cb_of):
    """`crafted` with any k11 <= cA per candidate: candidate j of item t is held by k11_of(D)[j] of the item's cA users (j, j + 1, ... modulo cA), fillers
    raise every column's count to cb_of(D)[j].  Returns ([A, B], rows) like crafted."""
    n_items = len(sizes)
    b_rows = [[] for _ in range(n_items * ca)]
    col0, rows, want = 0, [], []
    for t, D in enumerate(sizes):
        k11 = np.asarray(k11_of(D), np.int64)
        cb = np.maximum(np.asarray(cb_of(D), np.int64), k11)
        assert k11.size == D and cb.size == D and k11.min() >= 1 and k11.max() <= ca
        for j in range(D):
            for r in range(int(k11[j])):
                b_rows[t * ca + (j + r) % ca].append(col0 + j)
        rows.append((ca, k11, cb))
        want.append(cb - k11)
        col0 += D
    want = np.concatenate(want)
    n_fill = int(want.max())
    first_fill = n_items * ca
    assert first_fill + n_fill <= n_users
    all_rows = [np.sort(np.array(r, np.int64)) for r in b_rows] + [np.nonzero(want > f)[0] for f in range(n_fill)]
    a_rp = np.zeros(n_users + 1, np.int64)
    a_rp[1:first_fill + 1] = np.arange(1, first_fill + 1)
    a_rp[first_fill + 1:] = first_fill
    a = O.Csr(n_users, n_items, a_rp, np.repeat(np.arange(n_items), ca).astype(np.int32))
    lens_b = np.zeros(n_users, np.int64)
    lens_b[:len(all_rows)] = [r.size for r in all_rows]
    b_rp = np.zeros(n_users + 1, np.int64)
    np.cumsum(lens_b, out=b_rp[1:])
    return [a, O.Csr(n_users, col0, b_rp, np.concatenate(all_rows).astype(np.int32))], rows


def llr_of(sess, ca, k11, cb, n_users):
    """LLR of (k11, cA, cB) through the library under test (urcco_dev_llr: bit-identical to what the row kernels score)."""
    import torch
    k11, cb = np.asarray(k11, np.int64), np.asarray(cb, np.int64)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(sess.device)
    out = sess.llr(t(np.full(cb.size, int(ca), np.int64)), t(cb), t(k11), t(np.full(cb.size, int(n_users), np.int64)))
    sess.synchronize()
    return out.cpu().numpy()


def model_direct(rows, k, limit_of, n_cols, prefilter=True, valid_of=None):
    """Rows the direct ranking takes, by model_scored's rule for what the score phase sees: per row, the candidates the prefilter leaves (all of them with
    `prefilter` off), of those the valid ones (valid_of(ca, k11, cb) -> bool mask; default: every one -- N is large, every LLR positive), and the row counts
    when k < C <= the limit of ITS class.  Returns (rows taken, [(class, C)] per row)."""
    taken, seen = 0, []
    for ca, k11, cb in rows:
        keep = np.ones(k11.size, bool)
        if prefilter and k11.size > k:
            one = k11 == 1
            cum = np.cumsum(np.bincount(cb[one & (cb < CLAMP_BIN)], minlength=CLAMP_BIN))
            at = np.nonzero(cum >= k)[0]
            lim = limit_of(ca)
            if at.size and at[0] < lim:
                keep = ~(one & (cb > at[0]) & (cb <= lim))
        if valid_of is not None:
            keep &= valid_of(ca, k11, cb)
        c = class_of(int(k11.sum()), ca, n_cols, k)
        C = int(keep.sum())
        seen.append((c, C))
        taken += int(k < C <= DIRECT_LIMIT.get(c, 0))
    return taken, seen


def run_pair(sess, mats, params, seed, run=run_device, bits=0):
    """(with the direct ranking, without) outputs of the same build."""
    sess.set_debug(bits)
    try:
        on = run(sess, mats, params, seed)
        sess.set_debug(bits | _lib.DBG_NO_DIRECT_RANK)
        off = run(sess, mats, params, seed)
    finally:
        sess.set_debug(0)
    return on, off


def direct_rows(sess, mats, params, seed, run=run_device, bits=0):
    """stats[30] of every event type under COUNT_DIRECT: the rows that were ranked directly."""
    sess.set_timing(True)
    try:
        sess.set_debug(bits | _lib.DBG_COUNT_DIRECT)
        return [int(o.stats.cpu().numpy()[30]) for o in run(sess, mats, params, seed)]
    finally:
        sess.set_debug(0)
        sess.set_timing(False)


def check(sess, mats, params, seed=3, bits=0):
    """Oracle comparison (|dLLR| <= 1e-6, exact ids up to the k-boundary tie rule) of the build with the direct ranking, then on against off bit for bit.
    Returns the rows by accumulator class of every event type."""
    sess.set_debug(bits)
    try:
        _, _, stats = compare_with_oracle(sess, mats, params, seed)
    finally:
        sess.set_debug(0)
    on, off = run_pair(sess, mats, params, seed, bits=bits)
    assert_bit_equal(on, off)
    return [s[0][1:8] for s in stats]


def edge_case(c, k=50, multi=5):
    """Rows of class c around its limit: both sizes of the class, C = limit - 1, limit, limit + 1 (with `multi` k11 = 2 candidates each) -- and, with multi = 0,
    C = k and k + 1 (every survivor then is a k11 = 1 candidate at or below the cut)."""
    lim = DIRECT_LIMIT[c] or SEL_M[c]
    Cs = [k, k + 1] if multi == 0 else [lim - 1, lim, lim + 1]
    sizes = [D for D in CLASS_SIZES[c] for _ in Cs]
    mats, rows = crafted(np.random.default_rng(7), sizes, ca=4, n_users=N_BIG, cb_of=survivor_counts(k, multi=multi)(Cs * 2), multi=multi)
    return mats, rows, Cs * 2


def unordered_case(lib, device, mats, params, seed=3):
    """URCCO_FLAG_UNORDERED_ROWS (a context flag): rows are top-k SETS -- compared as sets, on against off and against the oracle; no row is ranked directly."""
    from universal_recommender_amd.device import Context, cross_occurrence_context
    ctx = Context(device, lib, flags=_lib.FLAG_UNORDERED_ROWS)
    try:
        def run(c, m, p, sd):
            out = cross_occurrence_context(c, [to_dev(x, device) for x in m], to_params(p), sd)
            return [type("Held", (), {"to_host": (lambda self, h=o.to_host(): h), "stats": o.stats.clone()})() for o in out]   # (a context reuses its output pool)
        on, off = run_pair(ctx, mats, params, seed, run)
        assert_bit_equal(on, off, as_sets=True)
        for o, r in zip(on, O.cross_occurrence_downsampled(mats, params, seed)):
            check_indicators(sort_rows(o.to_host()), r)
        assert direct_rows(ctx, mats, params, seed, run) == [0] * len(mats)
    finally:
        ctx.close()


# ---- the cases, run by both test files on their session -------------------------------------------------------------------------------------------
def P(k=50, min_llr=None, max_rows=100000):
    return O.DatasetParams(max_rows, k, min_llr)


def limit_fn(sess, n_users=N_BIG):
    from prefilter_cases import mono_limit
    cache = {}

    def limit_of(ca):
        if ca not in cache:
            cache[ca] = mono_limit(sess, ca, n_users)
        return cache[ca]
    return limit_of


def counted(sess, mats, rows, k, limit_of, bits=0, params=None, valid_of=None):
    """check(), then COUNT_DIRECT of A'B against the model.  Returns the model's (class, C) per row."""
    params = params or [P(k), P(k)]
    check(sess, mats, params, bits=bits)
    want, seen = model_direct(rows, k, limit_of, mats[1].n_cols, prefilter=not (bits & _lib.DBG_NO_PREFILTER), valid_of=valid_of)
    got = direct_rows(sess, mats, params, 3, bits=bits)
    print(f"rows ranked directly: {got} (model {want}); (class, C) per row: {seen}")
    assert got[1] == want, (got, want, seen)
    return want, seen


def case_edges(sess, c, multi):
    k = 50
    mats, rows, Cs = edge_case(c, k, multi)
    want, seen = counted(sess, mats, rows, k, limit_fn(sess))
    assert seen == [(c, C) for C in Cs], (seen, Cs)          # the rows are in the class, with the survivor counts, they were built for
    lim = DIRECT_LIMIT[c]
    assert want == sum(k < C <= lim for C in Cs)


def case_no_prefilter(sess):
    """NO_PREFILTER in both builds: the direct ranking ranks candidates the prefilter would have dropped.  One-wave rows of D = k + 1 and D = 64 (cA = 80:
    not the micro class) and rows of the 256-thread / 4Ki class with D at and one beyond its limit (k11 = cA = 12: 12 D > 512 pairs)."""
    k = 50
    mats, rows = crafted(np.random.default_rng(3), [k + 1, 64, 65], ca=80, n_users=N_BIG)
    _, seen = counted(sess, mats, rows, k, limit_fn(sess), bits=_lib.DBG_NO_PREFILTER)
    assert seen == [(1, k + 1), (1, 64), (1, 65)], seen
    lim = DIRECT_LIMIT[2] or SEL_M[2]
    rng = np.random.default_rng(4)
    mats, rows = general([lim, lim + 1, k + 1], 12, N_BIG, lambda D: np.full(D, 12), lambda D: rng.integers(12, 200, D))
    _, seen = counted(sess, mats, rows, k, limit_fn(sess), bits=_lib.DBG_NO_PREFILTER)
    assert seen == [(2, lim), (2, lim + 1), (2, k + 1)], seen


def case_ties(sess):
    """Every candidate the same count (all LLRs bit-equal: the row is cut by column alone), then two count values whose boundary falls exactly at rank k;
    with the prefilter in front (which keeps a tie at the cut whole, and drops the second value's candidates) and without."""
    k = 50
    for bits in (0, _lib.DBG_NO_PREFILTER):
        for cb_lo, cb_hi in ((7, 7), (3, 9)):
            def cb_of(rng, n, lo=cb_lo, hi=cb_hi):
                return np.where(np.arange(n) < k, lo, hi)
            mats, rows = crafted(np.random.default_rng(5), [60, 64], ca=80, n_users=N_BIG, cb_of=cb_of, multi=0)
            _, seen = counted(sess, mats, rows, k, limit_fn(sess), bits=bits)
            assert [c for c, _ in seen] == [1, 1], seen
            mats, rows = general([100, 128], 12, N_BIG, lambda D: np.full(D, 12), lambda D: np.where(np.arange(D) < k, cb_lo + 12, cb_hi + 12))
            _, seen = counted(sess, mats, rows, k, limit_fn(sess), bits=bits)
            assert seen == [(2, 100), (2, 128)], seen


def case_k(sess, k):
    """k = 64: C > k and C <= 64 exclude each other in the one-wave class; k = 65: it must never fire there."""
    mats, rows = crafted(np.random.default_rng(100 + k), [130, 400], ca=3, n_users=N_BIG)
    want, seen = counted(sess, mats, rows, k, limit_fn(sess))
    assert [c for c, _ in seen] == [1, 2], seen
    if k >= 64:
        assert want == int(k < seen[1][1] <= DIRECT_LIMIT[2]), (want, seen)
    else:
        assert want >= 1, (want, seen)


def case_min_llr(sess):
    """minLLR fails some survivors: C drops from above the limit to inside it.  20 candidates with k11 = 2, then k11 = 1 candidates with the counts
    1 .. 49, 50, 50, ... (the cut is at 50), the rest at 60 (dropped); minLLR sits between the scores of cB = 40 and cB = 41."""
    k, ca, m = 50, 4, 20
    S = {100: 60, 300: 130}       # k11 = 1 candidates at or below the cut: 80 survivors (one wave, limit 64), 150 (256 threads / 4Ki, limit 128)

    def cb_of(rng, n):
        cb = np.full(n, 60, np.int64)
        cb[:m] = 3
        cb[m:m + S[n]] = np.minimum(np.arange(1, S[n] + 1), k)
        return cb
    mats, rows = crafted(np.random.default_rng(9), [100, 300], ca=ca, n_users=N_BIG, cb_of=cb_of, multi=m)
    f = llr_of(sess, ca, [1, 1], [40, 41], N_BIG)
    thr = float((f[0] + f[1]) / 2)
    assert f[0] > thr > f[1]
    limit_of = limit_fn(sess)
    _, before = model_direct(rows, k, limit_of, mats[1].n_cols)
    assert before == [(1, 80), (2, 150)], before
    want, seen = counted(sess, mats, rows, k, limit_of, params=[P(k, thr), P(k, thr)], valid_of=lambda a, k11, cb: llr_of(sess, a, k11, cb, N_BIG) >= thr)
    assert seen == [(1, 60), (2, 60)], seen
    assert want == int(60 <= DIRECT_LIMIT[1]) + int(60 <= DIRECT_LIMIT[2])
    lens = np.diff(run_device(sess, mats, [P(k, thr), P(k, thr)], 3)[1].to_host()[0])
    assert lens.tolist() == [k, k], lens


def case_self_pair_and_unordered(sess, lib):
    """A'A with exclude_self on Zipf data (the self pair -- k11 = cA -- is among the prefilter's survivors of every row; its key is 0: it counts neither in C
    nor in the set), and URCCO_FLAG_UNORDERED_ROWS: the same sets, no row ranked directly."""
    from helpers import rand_csr
    rng = np.random.default_rng(31)
    a = rand_csr(rng, 60000, 3000, 6, zipf_s=1.1)
    b = rand_csr(rng, 60000, 9000, 14, zipf_s=1.0)
    bins = check(sess, [a, b], [P(20), P(20)])
    assert bins[0][1] > 0 and bins[0][2] > 0, bins
    got = direct_rows(sess, [a, b], [P(20), P(20)], 3)
    assert got[0] > 0 and got[1] > 0, got
    unordered_case(lib, sess.device, [a, b], [P(20), P(20)])
