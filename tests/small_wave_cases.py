"""Workloads and a plain-numpy model of the micro-shaped body of the one-wave class's small rows (csrc/cco_rows.hip, cco_rows_small_kernel), shared by
test_sim_small_wave.py and test_gpu_small_wave.py: with the class split (a build of >= URCCO_MICRO_SPLIT_ROWS item rows, k <= 63) a row of the one-wave class
with <= 64 users and <= 128 / <= 256 pairs runs two / four pairs per lane through the micro class's row body, the k11 = 1 prefilter in front of its tail; a row
that keeps more than 64 survivors takes the body's fallback.  Every case compares the build with the oracle and, bit for bit (row lengths, ids, LLR bits),
with the same build under NO_SMALL_WAVE; COUNT_SMALL_WAVE (stats[30] while stage timing is on: rows of the body, + 2^32 per fallback row) must report exactly
what the model of the sub-list rule names -- no case can pass with the path dead."""
import numpy as np

from direct_rank_cases import class_of
from helpers import check_indicators, compare_with_oracle, rand_csr, run_device, sort_rows, to_dev, to_params
from oracle import c_oracle as O
from prefilter_cases import CLAMP_BIN, assert_bit_equal, mono_limit
from universal_recommender_amd import _lib

N_BIG = 200_000            # users: cA cB << N for every candidate of the crafted rows
SMALL_KMAX = 63            # SMALL_KMAX of cco_rows.hip: beyond it the class keeps one list
MAX_USERS, MAX_PAIRS = 64, 256
OFF, COUNT = _lib.DBG_NO_SMALL_WAVE, _lib.DBG_COUNT_SMALL_WAVE


def P(k=50, min_llr=None, max_rows=100000):
    return O.DatasetParams(max_rows, k, min_llr)


def build(specs, n_users=N_BIG, seed=1):
    """specs[t] = (ca, n_hold, k11[D], cB[D]): item t of A is held by ca users who hold nothing else; n_hold of them -- drawn among the ca, so the others' EMPTY
    B' rows lie before, between and behind them -- deal out the row's D columns (fresh columns per item): candidate j sits in the rows of k11[j] of them.
    Filler users who hold no item of A raise every column's count to its cB.  Returns ([A, B], rows) with rows[t] = (ca, k11, cB) of A'B."""
    rng = np.random.default_rng(seed)
    b_rows, a_items, rows, want, col0 = [], [], [], [], 0
    for t, (ca, n_hold, k11, cb) in enumerate(specs):
        k11 = np.asarray(k11, np.int64)
        cb = np.maximum(np.asarray(cb, np.int64), k11)
        assert k11.size == cb.size and k11.min() >= 1 and k11.max() <= n_hold <= ca
        hold = np.sort(rng.choice(ca, n_hold, replace=False))
        mine = [[] for _ in range(ca)]
        for j in range(k11.size):
            for r in range(int(k11[j])):
                mine[hold[(j + r) % n_hold]].append(col0 + j)
        b_rows += mine
        a_items += [t] * ca
        rows.append((ca, k11, cb))
        want.append(cb - k11)
        col0 += k11.size
    want = np.concatenate(want)
    n_fill, first_fill = int(want.max()), len(b_rows)
    assert first_fill + n_fill <= n_users, "n_users too small for the fillers"
    all_rows = [np.sort(np.array(r, np.int64)) for r in b_rows] + [np.nonzero(want > f)[0] for f in range(n_fill)]
    a_rp = np.zeros(n_users + 1, np.int64)
    a_rp[1:first_fill + 1] = np.arange(1, first_fill + 1)
    a_rp[first_fill + 1:] = first_fill
    a = O.Csr(n_users, len(specs), a_rp, np.asarray(a_items, np.int32))
    lens = np.zeros(n_users, np.int64)
    lens[:len(all_rows)] = [r.size for r in all_rows]
    b_rp = np.zeros(n_users + 1, np.int64)
    np.cumsum(lens, out=b_rp[1:])
    return [a, O.Csr(n_users, col0, b_rp, np.concatenate(all_rows).astype(np.int32))], rows


def rows_of(a, b):
    """(cA, k11, cB) of every non-empty item row of A'B, from the (down-sampled) matrices."""
    a_cp, a_ri = O.transpose(a)
    cnt_b = O.column_counts(b)
    rows = []
    for i in np.nonzero(np.diff(a_cp))[0]:
        users = a_ri[a_cp[i]:a_cp[i + 1]]
        cols = np.concatenate([b.col_idx[b.row_ptr[u]:b.row_ptr[u + 1]] for u in users])
        uniq, k11 = np.unique(cols, return_counts=True)
        rows.append((int(users.size), k11.astype(np.int64), cnt_b[uniq].astype(np.int64)))
    return rows


def rows_of_build(mats, params, seed):
    ds = [O.downsample(m, O.column_counts(m), seed, p.max_elements_per_row, 0) for m, p in zip(mats, params)]
    return [rows_of(ds[0], b) for b in ds]


def model(rows, k, n_cols, limit_of, exclude_self=False, prefilter=True, split=True):
    """(rows of the body, rows of its fallback): a row of the one-wave class (choose_bin) with <= 64 users and <= 256 pairs, while the class is split and
    k <= SMALL_KMAX; its survivors are what the k11 = 1 prefilter leaves (prefilter_cases.model_scored's rule), and more than 64 of them take the fallback."""
    in_form = fallback = 0
    for ca, k11, cb in rows:
        w = int(k11.sum())
        if not (split and k <= SMALL_KMAX and w > 0 and class_of(w, ca, n_cols, k) == 1 and ca <= MAX_USERS and w <= MAX_PAIRS):
            continue
        in_form += 1
        D, need = k11.size, k + (1 if exclude_self else 0)
        surv = D
        if prefilter and D > need:
            one = k11 == 1
            at = np.nonzero(np.cumsum(np.bincount(cb[one & (cb < CLAMP_BIN)], minlength=CLAMP_BIN)) >= need)[0]
            lim = limit_of(ca)
            if at.size and at[0] < lim:
                surv = D - int((one & (cb > at[0]) & (cb <= lim)).sum())
        fallback += surv > 64
    return in_form, fallback


def limit_fn(sess, n_users=N_BIG):
    cache = {}

    def limit_of(ca):
        if ca not in cache:
            cache[ca] = mono_limit(sess, ca, n_users)
        return cache[ca]
    return limit_of


def run_pair(sess, mats, params, seed, run=run_device, bits=0):
    """(with the body, with its rows in the general kernel) outputs of the same build."""
    sess.set_debug(bits)
    try:
        on = run(sess, mats, params, seed)
        sess.set_debug(bits | OFF)
        off = run(sess, mats, params, seed)
    finally:
        sess.set_debug(0)
    return on, off


def small_rows(sess, mats, params, seed, run=run_device, bits=0):
    """stats[30] of every event type under COUNT_SMALL_WAVE: (rows of the body, rows of its fallback)."""
    sess.set_timing(True)
    try:
        sess.set_debug(bits | COUNT)
        words = [int(o.stats.cpu().numpy()[30]) for o in run(sess, mats, params, seed)]
    finally:
        sess.set_debug(0)
        sess.set_timing(False)
    return [(w & 0xffffffff, w >> 32) for w in words]


def check(sess, mats, params, seed=3, bits=0):
    sess.set_debug(bits)
    try:
        _, _, stats = compare_with_oracle(sess, mats, params, seed)
    finally:
        sess.set_debug(0)
    on, off = run_pair(sess, mats, params, seed, bits=bits)
    assert_bit_equal(on, off)
    return [s[0][1:8] for s in stats]


def counted(sess, mats, rows, k, limit_of=None, bits=0, params=None, seed=3):
    """check(), then COUNT_SMALL_WAVE of A'B against the model.  Returns the model's (rows of the body, rows of its fallback)."""
    params = params or [P(k), P(k)]
    check(sess, mats, params, seed, bits)
    want = model(rows, k, mats[1].n_cols, limit_of or limit_fn(sess, mats[0].n_rows), prefilter=not (bits & _lib.DBG_NO_PREFILTER))
    got = small_rows(sess, mats, params, seed, bits=bits)
    print(f"rows of the small-row body, of its fallback: {got} (model of A'B {want})")
    assert got[1] == want, (got, want)
    return want


def distinct(w, ca=4, cb_hi=120, seed=0):
    """a row of w pairs: w distinct columns, every k11 = 1, counts drawn from 1 .. cb_hi"""
    return (ca, ca, np.ones(w, np.int64), np.random.default_rng(seed + w).integers(1, cb_hi, w))


def repeated(w, ca=32, seed=0):
    """a row of w pairs over few columns: every column in the rows of all ca users but the last, which takes the remainder"""
    k11 = np.array([ca] * (w // ca) + ([w % ca] if w % ca else []), np.int64)
    return (ca, ca, k11, k11 + np.random.default_rng(seed + w).integers(0, 40, k11.size))


# ---- the cases, run by both test files on their session ---------------------------------------------------------------------------------------------
def case_pair_boundaries(sess):
    """Rows of exactly 64, 65, 128, 129, 256 and 257 pairs, all-distinct columns (D = w, every k11 = 1) and heavily repeated ones (few candidates, large
    k11): 64 is a micro row, 65 .. 128 and 129 .. 256 the two sub-lists, 257 stays in the general kernel."""
    k = 50
    ws = [64, 65, 128, 129, 256, 257]
    mats, rows = build([distinct(w) for w in ws] + [repeated(w) for w in ws])
    want = counted(sess, mats, rows, k)
    assert want[0] == 8, want          # 65, 128, 129, 256 of either make-up


def case_user_boundary(sess):
    """64 and 65 users at ~100 pairs, 40 of them with a B' row and the others' empty rows among them; and 64 users who all hold a pair."""
    k = 50
    rng = np.random.default_rng(2)
    spec = lambda ca, hold: (ca, hold, np.ones(100, np.int64), rng.integers(1, 90, 100))
    mats, rows = build([spec(64, 40), spec(65, 40), spec(64, 64), spec(65, 65), spec(63, 1)])
    want = counted(sess, mats, rows, k)
    assert want[0] == 3, want


def survivors_spec(D, s, k, multi, ca=4):
    """D candidates: `multi` with k11 = 2, then s with k11 = 1 and the counts 1 .. k - 1, k, k, ... (a tie at the cut, kept whole), the rest above the cut and
    inside the limit -- dropped.  multi + s survivors when s >= k."""
    k11 = np.ones(D, np.int64)
    k11[:multi] = 2
    cb = np.full(D, 80, np.int64)
    cb[:multi] = 3
    cb[multi:multi + s] = np.minimum(np.arange(1, s + 1), k)
    return (ca, ca, k11, cb)


def case_survivor_counts(sess):
    """k - 1 candidates in all (no cut), then k, k + 1, 64 and 65 survivors made by ties at the cut count -- 65 forces the fallback -- in rows of either sub-list."""
    k = 50
    specs = [(4, 4, np.array([2] * 20 + [1] * (k - 1 - 20)), np.arange(3, 3 + k - 1))]           # k - 1 candidates, 69 pairs
    for D in (120, 240):
        specs += [survivors_spec(D, k, k, 0), survivors_spec(D, k + 1, k, 0), survivors_spec(D, 59, k, 5), survivors_spec(D, 60, k, 5), survivors_spec(D, 64, k, 0),
                  survivors_spec(D, 65, k, 0)]
    mats, rows = build(specs)
    want = counted(sess, mats, rows, k)
    assert want == (13, 4), want       # per sub-list: 65 = 5 + 60 and 65 = 0 + 65 survivors


def case_nothing_pruned(sess):
    """Up to 256 survivors reach the fallback: (a) no prefilter in front (NO_PREFILTER in both builds); (b) a build of so few users that cA cB >= N early --
    the monotone limit of the row's cA lies at or below the cut and nothing is dropped.  (A row of this body holds <= 64 users: a cA beyond the xLogX table
    cannot be one of its rows.)"""
    k = 50
    mats, rows = build([distinct(65), distinct(128), distinct(200), distinct(256), repeated(256, 64)])
    want = counted(sess, mats, rows, k, bits=_lib.DBG_NO_PREFILTER)
    assert want == (5, 4), want
    n_users = 1500
    rng = np.random.default_rng(8)
    spec = lambda w: (60, 60, np.ones(w, np.int64), rng.integers(30, 60, w))
    mats, rows = build([spec(100), spec(256)], n_users=n_users)
    limit_of = limit_fn(sess, n_users)
    assert limit_of(60) <= 30, limit_of(60)        # (the G statistic falls with cB only while cA cB < N: cB < 25)
    want = counted(sess, mats, rows, k, limit_of)
    assert want == (2, 2), want


def case_k(sess, k):
    """k = 7, 50, 63: the sub-lists are built; k = 64 and 65: the class keeps one list (the fast tail ranks at most 64 survivors, and the prefilter keeps >= k)."""
    mats, rows = build([distinct(70, cb_hi=200), distinct(130, cb_hi=200), distinct(250, cb_hi=200), repeated(200)])
    want = counted(sess, mats, rows, k)
    assert want[0] == (4 if k <= SMALL_KMAX else 0), (k, want)


def case_min_llr(sess):
    """minLLR removes part of a row: the survivors with k11 = 1 and cB > 40 fail it."""
    from direct_rank_cases import llr_of
    k, ca = 50, 4
    mats, rows = build([survivors_spec(100, 60, k, 3), survivors_spec(250, 64, k, 3)])
    f = llr_of(sess, ca, [1, 1], [40, 41], N_BIG)
    thr = float((f[0] + f[1]) / 2)
    assert f[0] > thr > f[1]
    want = counted(sess, mats, rows, k, params=[P(k, thr), P(k, thr)])
    assert want == (2, 1), want
    lens = np.diff(run_device(sess, mats, [P(k, thr), P(k, thr)], 3)[1].to_host()[0])
    assert lens.tolist() == [43, 43], lens          # the 3 with k11 = 2 and the counts 1 .. 40


def zipf_pair(seed=31):
    rng = np.random.default_rng(seed)
    return [rand_csr(rng, 30000, 2500, 5, zipf_s=1.1), rand_csr(rng, 30000, 6000, 12, zipf_s=1.0)]


def counted_build(sess, mats, params, seed=3, bits=0):
    """check() and the counts of EVERY event type against the model of the down-sampled matrices (event 0 is A'A: the self pair is among its candidates)."""
    bins = check(sess, mats, params, seed, bits)
    limit_of = limit_fn(sess, mats[0].n_rows)
    want = [model(r, p.max_interesting_elements, m.n_cols, limit_of, exclude_self=(d == 0))
            for d, (r, p, m) in enumerate(zip(rows_of_build(mats, params, seed), params, mats))]
    got = small_rows(sess, mats, params, seed, bits=bits)
    print(f"rows by class {[b.tolist() for b in bins]}; rows of the small-row body, of its fallback {got} (model {want})")
    assert got == want, (got, want)
    return got


def case_self_pair_and_unordered(sess, lib):
    """A'A with the self pair excluded (it is one of the prefilter's counted candidates) and A'B without one, on Zipf data with rows of mixed sizes in one launch
    -- list ends and a short last group for the prefetch chain --; then URCCO_FLAG_UNORDERED_ROWS: the same sets."""
    from universal_recommender_amd.device import Context, cross_occurrence_context
    mats, params = zipf_pair(), [P(20), P(20)]
    got = counted_build(sess, mats, params)
    assert got[0][0] > 0 and got[1][0] > 0, got
    ctx = Context(sess.device, lib, flags=_lib.FLAG_UNORDERED_ROWS)
    try:
        def run(c, m, p, sd):
            out = cross_occurrence_context(c, [to_dev(x, sess.device) for x in m], to_params(p), sd)
            return [type("Held", (), {"to_host": (lambda self, h=o.to_host(): h), "stats": o.stats.clone()})() for o in out]   # (a context reuses its output pool)
        on, off = run_pair(ctx, mats, params, 3, run)
        assert_bit_equal(on, off, as_sets=True)
        for o, r in zip(on, O.cross_occurrence_downsampled(mats, params, 3)):
            check_indicators(sort_rows(o.to_host()), r)
        assert small_rows(ctx, mats, params, 3, run) == got
    finally:
        ctx.close()


def case_column_addressed(sess):
    """A B of 300 columns (<= the accumulator: slots are addressed by column), rows of both sub-lists."""
    rng = np.random.default_rng(41)
    mats = [rand_csr(rng, 4000, 400, 3, zipf_s=0.9), rand_csr(rng, 4000, 300, 10, zipf_s=0.7)]
    got = counted_build(sess, mats, [P(20), P(20)])
    assert got[1][0] > 0, got


def case_plain_form(sess):
    """(a) the packed and the plain form agree bit for bit: the same build under UNPACKED_COUNTS, where the whole class runs in the plain instantiation of the
    general kernel and the body counts no row; (b) a catalogue of 2^20 columns with a column held by 3000 users and no interaction cut: its count does not
    fit the word, the pack pass says so, and the plain form takes the whole class."""
    mats, rows = build([distinct(65), distinct(128), distinct(200), repeated(256)])
    params = [P(), P()]
    assert counted(sess, mats, rows, 50)[0] == 4
    on = run_device(sess, mats, params, 3)
    sess.set_debug(_lib.DBG_UNPACKED_COUNTS)
    try:
        plain = run_device(sess, mats, params, 3)
    finally:
        sess.set_debug(0)
    assert_bit_equal(on, plain)
    assert small_rows(sess, mats, params, 3, bits=_lib.DBG_UNPACKED_COUNTS) == [(0, 0), (0, 0)]
    rng = np.random.default_rng(61)
    n_users, n_cols = 4000, 1 << 20
    base = rand_csr(rng, n_users, n_cols, 8)
    hot = np.zeros(n_users, bool)
    hot[rng.choice(n_users, 3000, replace=False)] = True
    brows = [np.unique(np.concatenate([base.col_idx[base.row_ptr[u]:base.row_ptr[u + 1]], [12345] if hot[u] else []]).astype(np.int32)) for u in range(n_users)]
    rp = np.zeros(n_users + 1, np.int64)
    np.cumsum([len(r) for r in brows], out=rp[1:])
    wide = O.Csr(n_users, n_cols, rp, np.concatenate(brows))
    assert O.column_counts(wide)[12345] >= 2048
    prim = rand_csr(rng, n_users, 300, 6, zipf_s=0.8)
    mats, params = [prim, wide], [P(), P()]
    bins = check(sess, mats, params, 23)
    in_range = sum(1 for ca, k11, _ in rows_of_build(mats, params, 23)[1] if ca <= MAX_USERS and 64 < int(k11.sum()) <= MAX_PAIRS)
    assert bins[1][1] > 0 and in_range > 0, (bins, in_range)       # rows the body would take, had the counts fitted
    assert small_rows(sess, mats, params, 23)[1] == (0, 0)
