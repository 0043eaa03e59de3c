"""Workloads and a plain-numpy model of the small-row body with eight pairs and two users per lane (csrc/cco_rows.hip, cco_rows_small_kernel<8, 2>), shared by
test_sim_block_small_wave.py and test_gpu_block_small_wave.py.  With the classes split (a build of >= URCCO_MICRO_SPLIT_ROWS item rows, k <= 63, packed B') two
sub-lists run in that body: LIST 1, the rows of the one-wave class (bin 1) with <= 128 users that its two older sub-lists (<= 64 users and <= 256 pairs) leave;
LIST 2, the rows of the small-block class (bin 2) with <= 128 users and <= 512 pairs.  A row that keeps more than 64 survivors takes the body's fallback.
Every case compares the build with the oracle and, bit for bit (row lengths, ids in order, LLR bits), with the same build under NO_BLOCK_SMALL_WAVE;
COUNT_BLOCK_SMALL_WAVE (stats[30] while stage timing is on: rows of the body, + 2^32 per fallback row; URCCO_COUNT_BLOCK_LIST = 1 / 2 names one list) must
report exactly what the model of the sub-list rule names, per list -- no case can pass with the path dead."""
import os

import numpy as np

from direct_rank_cases import class_of
from helpers import check_indicators, compare_with_oracle, rand_csr, run_device, sort_rows, to_dev, to_params
from oracle import c_oracle as O
from prefilter_cases import CLAMP_BIN, assert_bit_equal
from small_wave_cases import N_BIG, P, SMALL_KMAX, distinct, limit_fn, repeated, rows_of_build, survivors_spec
from universal_recommender_amd import _lib

OFF, COUNT = _lib.DBG_NO_BLOCK_SMALL_WAVE, _lib.DBG_COUNT_BLOCK_SMALL_WAVE
MAX_USERS, MAX_PAIRS = 128, 512       # of the body: two users and eight pairs per lane
OLD_USERS, OLD_PAIRS = 64, 256        # of the one-wave class's two older sub-lists
LIST_ENV = "URCCO_COUNT_BLOCK_LIST"


def build(specs, n_users=N_BIG, seed=1):
    """small_wave_cases.build with the holders named: specs[t] = (ca, hold, k11[D], cB[D]) -- item t of A is held by ca users who hold nothing else; `hold` is
    how many of them (drawn among the ca, so the others' EMPTY B' rows lie before, between and behind them) or WHICH of them (positions in the row) deal out
    the row's D columns: candidate j sits in the rows of k11[j] of them.  Fillers raise every column's count to its cB.  Returns ([A, B], rows)."""
    rng = np.random.default_rng(seed)
    b_rows, a_items, rows, want, col0 = [], [], [], [], 0
    for t, (ca, hold, k11, cb) in enumerate(specs):
        k11 = np.asarray(k11, np.int64)
        hold = np.sort(rng.choice(ca, hold, replace=False)) if np.isscalar(hold) else np.asarray(hold, np.int64)
        n_hold = hold.size
        cb = np.maximum(np.asarray(cb, np.int64), k11)
        assert k11.size == cb.size and k11.min() >= 1 and k11.max() <= n_hold <= ca and hold.max() < ca
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


def list_of(w, ca, n_cols, k):
    """The sub-list rule (internal_bin of cco_rows.hip): 1, 2 or 0 = none of the two."""
    c = class_of(w, ca, n_cols, k)
    if c == 1 and ca <= MAX_USERS and not (ca <= OLD_USERS and w <= OLD_PAIRS):
        return 1
    if c == 2 and ca <= MAX_USERS and w <= MAX_PAIRS:
        return 2
    return 0


def model(rows, k, n_cols, limit_of, exclude_self=False, prefilter=True, split=True):
    """((rows of the body, rows of its fallback) of list 1, the same of list 2): the survivors of a row are what the k11 = 1 prefilter leaves
    (prefilter_cases.model_scored's rule), and more than 64 of them take the fallback."""
    got = {1: [0, 0], 2: [0, 0]}
    for ca, k11, cb in rows:
        w = int(k11.sum())
        which = list_of(w, ca, n_cols, k) if (split and k <= SMALL_KMAX and w > 0) else 0
        if not which:
            continue
        D, need = k11.size, k + (1 if exclude_self else 0)
        surv = D
        if prefilter and D > need:
            one = k11 == 1
            at = np.nonzero(np.cumsum(np.bincount(cb[one & (cb < CLAMP_BIN)], minlength=CLAMP_BIN)) >= need)[0]
            lim = limit_of(ca)
            if at.size and at[0] < lim:
                surv = D - int((one & (cb > at[0]) & (cb <= lim)).sum())
        got[which][0] += 1
        got[which][1] += surv > 64
    return tuple(got[1]), tuple(got[2])


def run_pair(sess, mats, params, seed, run=run_device, bits=0):
    """(with the two sub-lists in the body, with them in the general kernels) outputs of the same build."""
    sess.set_debug(bits)
    try:
        on = run(sess, mats, params, seed)
        sess.set_debug(bits | OFF)
        off = run(sess, mats, params, seed)
    finally:
        sess.set_debug(0)
    return on, off


def body_rows(sess, mats, params, seed, run=run_device, bits=0):
    """stats[30] of every event type under COUNT_BLOCK_SMALL_WAVE, per list: [((rows, fallback rows) of list 1, of list 2)]; the build that counts both lists
    together must report their sum."""
    saved = os.environ.pop(LIST_ENV, None)
    words = {}
    sess.set_timing(True)
    try:
        sess.set_debug(bits | COUNT)
        for which in ("1", "2", None):
            if which:
                os.environ[LIST_ENV] = which
            else:
                os.environ.pop(LIST_ENV, None)
            words[which] = [int(o.stats.cpu().numpy()[30]) for o in run(sess, mats, params, seed)]
    finally:
        sess.set_debug(0)
        sess.set_timing(False)
        os.environ.pop(LIST_ENV, None)
        if saved is not None:
            os.environ[LIST_ENV] = saved
    assert [a + b for a, b in zip(words["1"], words["2"])] == words[None], words
    split = lambda w: (w & 0xffffffff, w >> 32)
    return [(split(a), split(b)) for a, b in zip(words["1"], words["2"])]


def check(sess, mats, params, seed=3, bits=0):
    """Oracle comparison of the build with the body, then on against off bit for bit.  Returns the rows by accumulator class of every event type."""
    sess.set_debug(bits)
    try:
        _, _, stats = compare_with_oracle(sess, mats, params, seed)
    finally:
        sess.set_debug(0)
    on, off = run_pair(sess, mats, params, seed, bits=bits)
    assert_bit_equal(on, off)
    return [s[0][1:8] for s in stats]


def counted(sess, mats, rows, k, limit_of=None, bits=0, params=None, seed=3):
    """check(), then COUNT_BLOCK_SMALL_WAVE of A'B against the model.  Returns the model's ((rows, fallback) of list 1, of list 2)."""
    params = params or [P(k), P(k)]
    check(sess, mats, params, seed, bits)
    want = model(rows, k, mats[1].n_cols, limit_of or limit_fn(sess, mats[0].n_rows), prefilter=not (bits & _lib.DBG_NO_PREFILTER))
    got = body_rows(sess, mats, params, seed, bits=bits)
    print(f"rows of the body, of its fallback, per list: {got} (model of A'B {want})")
    assert got[1] == want, (got, want)
    return want


def counted_build(sess, mats, params, seed=3, bits=0):
    """check() and the counts of EVERY event type against the model of the down-sampled matrices (event 0 is A'A: the self pair is among its candidates)."""
    bins = check(sess, mats, params, seed, bits)
    limit_of = limit_fn(sess, mats[0].n_rows)
    want = [model(r, p.max_interesting_elements, m.n_cols, limit_of, exclude_self=(d == 0))
            for d, (r, p, m) in enumerate(zip(rows_of_build(mats, params, seed), params, mats))]
    got = body_rows(sess, mats, params, seed, bits=bits)
    print(f"rows by class {[b.tolist() for b in bins]}; rows of the body, of its fallback, per list {got} (model {want})")
    assert got == want, (got, want)
    return got


def spread(w, ca, hold, cb_hi=120, seed=0):
    """a row of w pairs, w distinct columns with k11 = 1, dealt out by `hold` of the row's ca users"""
    return (ca, hold, np.ones(w, np.int64), np.random.default_rng(seed + w + ca).integers(1, cb_hi, w))


# ---- the cases, run by both test files on their session ---------------------------------------------------------------------------------------------
def case_user_boundaries(sess):
    """64, 65, 127, 128 and 129 users at 100 pairs (one-wave class: 64 belongs to an older sub-list, 129 stays in the general kernel) and at 400 pairs
    (small-block class: 129 stays in the block kernel), 40 of the users with a B' row and the others' empty rows before, between and behind them; rows whose
    every user holds a pair; a row of 128 users whose only holders are users 64 .. 127, one whose only holder is user 127, one whose holders are 0 and 127."""
    k = 50
    specs = [spread(w, ca, 40) for w in (100, 400) for ca in (64, 65, 127, 128, 129)]
    specs += [spread(w, ca, ca) for w in (150, 400) for ca in (65, 128)]
    specs += [spread(w, 128, np.arange(64, 128)) for w in (120, 380)]
    specs += [spread(200, 128, np.array([127])), spread(300, 128, np.array([0, 127])), spread(90, 100, np.array([64]))]
    mats, rows = build(specs)
    want = counted(sess, mats, rows, k)
    assert want[0][0] == 3 + 2 + 1 + 2 and want[1][0] == 4 + 2 + 1 + 1, want


def case_pair_boundaries(sess):
    """Pairs around every edge of the rule, all-distinct columns (D = w: the accumulator's worst load at 512) and heavily repeated ones: 256 | 257 (older
    sub-list | list 1), 290 | 291 at k = 50 (the capacity edge: one-wave | small-block class), 511, 512 | 513 (list 2 | the block kernel)."""
    k = 50
    ws = [256, 257, 290, 291, 511, 512, 513]
    mats, rows = build([distinct(w) for w in ws] + [repeated(w) for w in ws] + [repeated(w, 64) for w in (257, 512)])
    want = counted(sess, mats, rows, k)
    assert want[0][0] == 2 + 2 + 1 and want[1][0] == 3 + 3 + 1, want
    assert any(k11.size == 512 and int(k11.sum()) == 512 for _, k11, _ in rows)


def case_survivor_counts(sess):
    """63, 64 and 65 survivors made by ties at the cut count (fast tail | fallback), with and without k11 = 2 candidates among them, in rows of both lists."""
    k = 50
    specs = []
    for D in (280, 480):
        specs += [survivors_spec(D, s, k, 0) for s in (63, 64, 65)] + [survivors_spec(D, s, k, 5) for s in (58, 59, 60)]
    mats, rows = build(specs)
    want = counted(sess, mats, rows, k)
    assert want == ((6, 2), (6, 2)), want


def case_fallback_shapes(sess):
    """The fallback's own paths, in rows of both lists.  (a) nothing pruned: every count beyond the histogram's clamp bin, so that all D <= 512 candidates are
    staged and scored; (b) all ties at the cut: every candidate the same count -- all keys equal, no digit cut, every survivor ranked against all; (c) two
    count values, 30 candidates of the better one: the digit cut's bin holds the 200 / 400 others, more than 64; (d) the same without a prefilter in front."""
    k = 50
    rng = np.random.default_rng(12)
    specs = []
    for D in (270, 500):
        specs += [(4, 4, np.ones(D, np.int64), rng.integers(CLAMP_BIN + 1, 400, D)),
                  (4, 4, np.ones(D, np.int64), np.full(D, 7)),
                  (4, 4, np.ones(D, np.int64), np.where(np.arange(D) < 30, 3, 9))]
    mats, rows = build(specs)
    assert counted(sess, mats, rows, k) == ((3, 3), (3, 3))
    assert counted(sess, mats, rows, k, bits=_lib.DBG_NO_PREFILTER) == ((3, 3), (3, 3))


def case_k(sess, k):
    """k = 1, 7, 50, 63: the sub-lists are built (which rows they hold follows the capacity rule of that k); k = 64 and 65: the classes keep one list each."""
    mats, rows = build([spread(150, 100, 60, cb_hi=200), distinct(280, cb_hi=200), distinct(400, cb_hi=200), repeated(500, 100), spread(330, 128, 128, cb_hi=200)])
    want = counted(sess, mats, rows, k)
    if k <= SMALL_KMAX:
        assert want[0][0] + want[1][0] == 5 and want[0][0] >= 1 and want[1][0] >= 2, (k, want)
    else:
        assert want == ((0, 0), (0, 0)), (k, want)


def case_min_llr(sess):
    """minLLR removes part of a row: the survivors with k11 = 1 and cB > 40 fail it, in a row of either list, fast tail and fallback."""
    from direct_rank_cases import llr_of
    k, ca = 50, 4
    mats, rows = build([survivors_spec(280, 60, k, 3), survivors_spec(480, 64, k, 3)])
    f = llr_of(sess, ca, [1, 1], [40, 41], N_BIG)
    thr = float((f[0] + f[1]) / 2)
    assert f[0] > thr > f[1]
    want = counted(sess, mats, rows, k, params=[P(k, thr), P(k, thr)])
    assert want == ((1, 0), (1, 1)), want
    lens = np.diff(run_device(sess, mats, [P(k, thr), P(k, thr)], 3)[1].to_host()[0])
    assert lens.tolist() == [43, 43], lens          # the 3 with k11 = 2 and the counts 1 .. 40


def zipf_pair(seed=33):
    """items of A held by up to a few hundred users, B' rows of a few entries: rows of 65 .. 128 users with <= 512 pairs in both event types"""
    rng = np.random.default_rng(seed)
    return [rand_csr(rng, 30000, 1500, 4, zipf_s=0.9), rand_csr(rng, 30000, 6000, 4, zipf_s=1.0)]


def case_self_pair_and_unordered(sess, lib):
    """A'A with the self pair excluded (it is one of the prefilter's counted candidates) and A'B without one, on Zipf data with rows of mixed sizes in one launch
    -- list ends and a short last group for the prefetch chain --; then URCCO_FLAG_UNORDERED_ROWS: the same sets."""
    from universal_recommender_amd.device import Context, cross_occurrence_context
    mats, params = zipf_pair(), [P(20), P(20)]
    got = counted_build(sess, mats, params)
    assert all(g[0][0] > 0 and g[1][0] > 0 for g in got), got
    ctx = Context(sess.device, lib, flags=_lib.FLAG_UNORDERED_ROWS)
    try:
        def run(c, m, p, sd):
            out = cross_occurrence_context(c, [to_dev(x, sess.device) for x in m], to_params(p), sd)
            return [type("Held", (), {"to_host": (lambda self, h=o.to_host(): h), "stats": o.stats.clone()})() for o in out]   # (a context reuses its output pool)
        on, off = run_pair(ctx, mats, params, 3, run)
        assert_bit_equal(on, off, as_sets=True)
        for o, r in zip(on, O.cross_occurrence_downsampled(mats, params, 3)):
            check_indicators(sort_rows(o.to_host()), r)
        assert body_rows(ctx, mats, params, 3, run) == got
    finally:
        ctx.close()


def case_column_addressed(sess):
    """A B of 900 columns (<= the accumulator's 1024 words: slots are addressed by column, and beyond the 512 of the older sub-lists), rows of both lists."""
    rng = np.random.default_rng(43)
    mats = [rand_csr(rng, 6000, 150, 3, zipf_s=0.8), rand_csr(rng, 6000, 900, 4, zipf_s=0.7)]
    got = counted_build(sess, mats, [P(20), P(20)])
    assert got[1][0][0] > 0 and got[1][1][0] > 0, got


def case_plain_form(sess):
    """(a) the packed and the plain form agree bit for bit: the same build under UNPACKED_COUNTS, where the whole classes run in the plain instantiations of the
    general kernels and the body counts no row; (b) a catalogue of 2^20 columns with a column held by 3000 users and no interaction cut: its count does not
    fit the word, the pack pass says so, and the plain form takes the whole classes."""
    mats, rows = build([spread(150, 100, 60), distinct(280), distinct(400), repeated(512, 100)])
    params = [P(), P()]
    want = counted(sess, mats, rows, 50)
    assert want[0][0] == 2 and want[1][0] == 2, want
    on = run_device(sess, mats, params, 3)
    sess.set_debug(_lib.DBG_UNPACKED_COUNTS)
    try:
        plain = run_device(sess, mats, params, 3)
    finally:
        sess.set_debug(0)
    assert_bit_equal(on, plain)
    none = ((0, 0), (0, 0))
    assert body_rows(sess, mats, params, 3, bits=_lib.DBG_UNPACKED_COUNTS) == [none, none]
    rng = np.random.default_rng(63)
    n_users, n_cols = 4000, 1 << 20
    base = rand_csr(rng, n_users, n_cols, 4)
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
    in_range = [sum(1 for ca, k11, _ in rows_of_build(mats, params, 23)[1] if list_of(int(k11.sum()), ca, n_cols, 50) == which) for which in (1, 2)]
    assert bins[1][1] > 0 and bins[1][2] > 0 and min(in_range) > 0, (bins, in_range)       # rows the body would take, had the counts fitted
    assert body_rows(sess, mats, params, 23)[1] == none


def case_counting_bits(sess):
    """The older counting bits on a build that mixes every list: COUNT_DIRECT, COUNT_SCORED (and the distinct candidates of a plain build) and COUNT_SMALL_WAVE
    report what their own models (direct_rank_cases, prefilter_cases, small_wave_cases) name -- the rows of the new sub-lists count as rows of their classes
    there, and not at all in COUNT_SMALL_WAVE."""
    import direct_rank_cases as DR
    import prefilter_cases as PF
    import small_wave_cases as SW
    k = 50
    specs = [distinct(100), distinct(200), spread(150, 100, 60), distinct(280), spread(280, 4, 4, cb_hi=300), survivors_spec(280, 70, k, 5)]
    specs += [distinct(400), spread(400, 128, 90, cb_hi=300), survivors_spec(480, 100, k, 5), survivors_spec(480, 130, k, 5), distinct(600), survivors_spec(900, 100, k, 5)]
    mats, rows = build(specs)
    params = [P(k), P(k)]
    limit_of = limit_fn(sess)
    want = counted(sess, mats, rows, k, limit_of)
    assert want[0][0] == 4 and want[1][0] == 4, want
    direct, seen = DR.model_direct(rows, k, limit_of, mats[1].n_cols)
    assert direct >= 2 and (2, 105) in seen, (direct, seen)               # rows of list 2 among them: 100 + 5 survivors
    assert DR.direct_rows(sess, mats, params, 3)[1] == direct, seen
    scored, plain = PF.scored_and_distinct(sess, mats, params, 3, run_device)
    assert (scored[1], plain[1]) == PF.model_scored(rows, k, limit_of), (scored, plain)
    small = SW.model(rows, k, mats[1].n_cols, limit_of)
    assert small[0] == 2, small
    assert SW.small_rows(sess, mats, params, 3)[1] == small
