"""Workloads for the whole k domain of the row kernels (csrc/cco_rows.hip), shared by test_sim_large_k.py and test_gpu_large_k.py: maxInterestingElements
far beyond a wave -- the capacity edges of the five LDS classes (choose_bin: 3 min(w, n_cols_b) + 3 k + 2 <= E), rows between the edges with mixed k11, and
the dense global kernel on both sides of GSEL_K = 1024 (radix select with full survivor arrays; the k strictly descending argmax sweeps beyond).

Every case goes through helpers.compare_with_oracle (pairs, the overflow word, row lengths, ids, |dLLR| <= helpers.LLR_TOL against oracle/c_oracle) and
asserts the accumulator class of EVERY row of the last event type from the statistics (stats[1 + bin]): a case that lands in another class fails.
`repeat` (the hardware driver): the build runs twice and the two outputs must be byte-identical."""
import numpy as np

import test_sim_kernel_logic as logic
from helpers import check_indicators, compare_with_oracle, run_device, sort_rows, to_dev, to_params
from oracle import c_oracle as O
from universal_recommender_amd import _lib

TABLE_WORDS = (1024, 4096, 8192, 16384, 32768)   # E of the classes 1 .. 5 (cco_rows.hip: E0, E1S, E1, E2S, E2)
GSEL_K = 1024                                    # cco_rows.hip: largest k of the radix select of the dense global kernel
DENSE = 6                                        # bin 6 at k > MP_KMAX = 256: the dense global kernel
MAX_ROWS = 100000                                # maxElementsPerRow: no row of these workloads is down-sampled


def P(k, min_llr=None):
    return O.DatasetParams(MAX_ROWS, k, min_llr)


def edge_of(E):
    """(s, k): the largest D + k a table of E words admits, and the largest k at which a row of that class can still be cut (D = s - k > k)."""
    return (E - 2) // 3, (E - 5) // 6


def class_of(w, ca, n_cols, k):
    """choose_bin of cco_rows.hip for rows whose counts fit the packed field (written out again here: the tests' expectation, not the library's)."""
    if w <= 64 and ca <= 64:
        return 0
    dmax = 3 * min(w, n_cols) + 3 * k + 2
    cap = next((c + 1 for c, E in enumerate(TABLE_WORDS) if dmax <= E), 6)
    return max(cap, 1 if w <= 512 else (2 if w <= 8192 else 4))


def one_row(cls):
    rows = [0] * 7
    rows[cls] = 1
    return rows


def assert_same_bytes(x, y, what):
    for u, v in zip(x, y):
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), f"{what}: two runs of the same build differ"


def checked(sess, mats, k, want, min_llr=None, item_hi=None, exact_ids=False, bits=0, repeat=False, seed=5):
    """compare_with_oracle, the rows by accumulator class of the LAST event type == want, and (repeat) a second, byte-identical run.
    Returns (host outputs per event type, oracle rows per event type)."""
    params = [P(k, min_llr)] * len(mats)
    sess.set_debug(bits)
    try:
        out, ref, stats = compare_with_oracle(sess, mats, params, seed, 0, 0, item_hi, exact_ids=exact_ids)
        hosts = [o.to_host() for o in out]
        if repeat:
            for d, (h, o2) in enumerate(zip(hosts, run_device(sess, mats, params, seed, 0, 0, item_hi))):
                assert_same_bytes(h, o2.to_host(), f"event {d}")
    finally:
        sess.set_debug(0)
    rows = stats[-1][0][1:8].tolist()
    print(f"k = {k}: rows by class {rows}, row lengths {np.diff(hosts[-1][0]).tolist()[:8]}")
    assert rows == want, (k, rows, want)
    return hosts, ref


def lens_of(ref):
    return np.diff(ref.to_csr()[0])


# ---- 1. capacity edges of the five LDS classes ----------------------------------------------------------------------------------------------------
N_BACK = 30


def _background(rng, first, n_cols):
    """(users, cols) of the N_BACK background users from `first` on: between n_cols / 8 and n_cols / 2 random columns each, so that cB varies."""
    users, cols = [], []
    for u in range(first, first + N_BACK):
        n = int(rng.integers(max(n_cols // 8, 1), max(n_cols // 2, 1) + 1))
        users.append(np.full(n, u, np.int64))
        cols.append(rng.choice(n_cols, n, replace=False))
    return users, cols


def hashed_row(D, n_cols=40_000, seed=1):
    """Item 0 is held by ONE user whose B row has D distinct columns out of n_cols (w = D: the hashed table; every candidate k11 = 1); the background
    users hold item 1.  [A, B]."""
    rng = np.random.default_rng(seed)
    users, cols = _background(rng, 1, n_cols)
    users.append(np.zeros(D, np.int64))
    cols.append(rng.choice(n_cols, D, replace=False))
    n_users = 1 + N_BACK
    a = logic.csr_from_pairs(n_users, 2, np.arange(n_users), np.concatenate([[0], np.ones(N_BACK, np.int64)]))
    return [a, logic.csr_from_pairs(n_users, n_cols, np.concatenate(users), np.concatenate(cols))]


def column_row(D, seed=2):
    """Two holders of item 0 each hold EVERY column of a B exactly D wide (n_cols_b = D < w = 2 D: the column-addressed table; k11 = 2 everywhere, the
    prefilter never fires); the background users hold item 1.  [A, B]."""
    rng = np.random.default_rng(seed)
    users, cols = _background(rng, 2, D)
    for u in (0, 1):
        users.append(np.full(D, u, np.int64))
        cols.append(np.arange(D))
    n_users = 2 + N_BACK
    a = logic.csr_from_pairs(n_users, 2, np.arange(n_users), np.concatenate([[0, 0], np.ones(N_BACK, np.int64)]))
    return [a, logic.csr_from_pairs(n_users, D, np.concatenate(users), np.concatenate(cols))]


def case_edge(sess, E, family, which, k=None, repeat=False):
    """One row of item 0 (item range [0, 1)) around the capacity edge of the class with E table words; k defaults to the largest at which the class still
    cuts a row.  which: "edge" (D + k = s: the class of E), "above" (D + k = s + 1: the next class -- the dense global kernel behind E = 32768),
    "edge_no_prefilter" (the hashed edge with every candidate through the compaction, the score phase and the select: the table completely full),
    "edge_k-1" (the edge at k - 1, D + 1: the other parity of D -- an odd D costs the key array's alignment word, 3 (D + k) + 1 words in all),
    "uncut" (D + k = s with D < k: the row keeps every candidate)."""
    cls = 1 + TABLE_WORDS.index(E)
    s, k_edge = edge_of(E)
    if which == "uncut":
        D = 70 if family == "hashed" else 40     # hashed: w = D > 64 (not the micro class); column-addressed: w = 2 D
        k = s - D
    else:
        k = (k_edge if k is None else k) - (which == "edge_k-1")
        D = s - k + (1 if which == "above" else 0)
    assert 3 * (D + k - (which == "above")) + 2 <= E < 3 * (D + k + (which != "above")) + 2      # on the edge / one above it
    mats = hashed_row(D) if family == "hashed" else column_row(D)
    w, ca = (D, 1) if family == "hashed" else (2 * D, 2)
    want = cls + 1 if which == "above" else cls
    assert class_of(w, ca, mats[1].n_cols, k) == want, (E, family, which, D, k)
    bits = _lib.DBG_NO_PREFILTER if which == "edge_no_prefilter" else 0
    _, ref = checked(sess, mats, k, one_row(want), item_hi=1, exact_ids=True, bits=bits, repeat=repeat)
    n = int(lens_of(ref[1])[0])
    assert n == min(D, k), (n, D, k)             # the oracle's row: every candidate valid, so the row is cut exactly when D > k
    return D, k


# ---- 2. rows between the edges, mixed k11 ---------------------------------------------------------------------------------------------------------
# (holders of item 0, n_cols, columns per holder, k, class of item 0's row, class of item 1's row or None: item range [0, 1))
MIXED = [(3, 3000, 500, 600, 3, 4),
         (3, 6000, 700, 1024, 4, 5), (3, 6000, 700, 1025, 4, 5), (3, 6000, 700, 1364, 4, 5),
         (2, 40000, 3000, 2729, 5, None),
         (2, 40000, 6000, 5460, 6, None), (2, 40000, 6000, 5461, 6, None),
         (2, 40000, 12000, 10922, 6, None)]


def mixed_row(holders, n_cols, per, seed=3):
    """Item 0 is held by `holders` users with random, overlapping B rows of `per` columns (k11 = 1 .. holders); 40 background users hold n_cols / 3 columns
    each, the first 10 of them hold item 1."""
    rng = np.random.default_rng(seed)
    n_users = holders + 40
    a = logic.csr_from_pairs(n_users, 2, np.arange(holders + 10), np.concatenate([np.zeros(holders, np.int64), np.ones(10, np.int64)]))
    users = [np.full(per, u, np.int64) for u in range(holders)] + [np.full(n_cols // 3, u, np.int64) for u in range(holders, n_users)]
    cols = [rng.choice(n_cols, per, replace=False) for _ in range(holders)] + [rng.choice(n_cols, n_cols // 3, replace=False) for _ in range(40)]
    return [a, logic.csr_from_pairs(n_users, n_cols, np.concatenate(users), np.concatenate(cols))]


# the simulator's twins of the last three (k argmax sweeps each): the same k on a catalogue whose rows have fewer candidates than k
MIXED_SMALL = [(2, 1200, 500, 5460, 5, None), (2, 1200, 500, 5461, 5, None), (2, 1200, 500, 10922, 6, None)]


def case_mixed(sess, holders, n_cols, per, k, cls0, cls1, repeat=False, cut=True):
    """Item 0's row (w = holders x per, cut: its distinct candidates outnumber k) and, where cls1 is given, item 1's (w = 10 n_cols / 3, nearly every column a
    candidate); at 40 000 columns item 1's row would be k argmax sweeps over 39 000 candidates and is left out by the item range."""
    mats = mixed_row(holders, n_cols, per)
    assert class_of(holders * per, holders, n_cols, k) == cls0
    want = one_row(cls0)
    if cls1 is not None:
        assert class_of(10 * (n_cols // 3), 10, n_cols, k) == cls1
        want[cls1] += 1
    _, ref = checked(sess, mats, k, want, item_hi=None if cls1 is not None else 1, repeat=repeat)
    lens = lens_of(ref[1])
    assert (lens[0] == k) if cut else (0 < lens[0] < k), (lens, k)       # the oracle's row: really cut (the small twins: not at all)
    return lens


# ---- 3. the dense global kernel on both sides of GSEL_K ---------------------------------------------------------------------------------------------
def dense_problem(n_cols=12_000, big=5000, small=300, seed=4):
    """B n_cols wide, 40 users: users 0 .. 15 hold `big` random columns each (users 0 .. 3 also the columns 0, 1, 2: the rows of B'B the self-pair case
    computes are heavy), the rest `small` each.  A has 3 items: users 0 .. 3 hold item 0, 4 .. 15 item 1, 16 .. 39 item 2."""
    rng = np.random.default_rng(seed)
    users = [np.full(big if u < 16 else small, u, np.int64) for u in range(40)] + [np.repeat(np.arange(4), 3)]
    cols = [rng.choice(n_cols, big if u < 16 else small, replace=False) for u in range(40)] + [np.tile(np.arange(3), 4)]
    a = logic.csr_from_pairs(40, 3, np.arange(40), np.concatenate([np.zeros(4, np.int64), np.ones(12, np.int64), np.full(24, 2, np.int64)]))
    return [a, logic.csr_from_pairs(40, n_cols, np.concatenate(users), np.concatenate(cols))]


def dense_classes(mats, k):
    """Rows by class of A'B for dense_problem, by the rule."""
    a, b = mats
    lens_b = np.diff(b.row_ptr)
    rows = [0] * 7
    for lo, hi in ((0, 4), (4, 16), (16, 40)):
        rows[class_of(int(lens_b[lo:hi].sum()), hi - lo, b.n_cols, k)] += 1
    return rows


def case_dense(sess, k, min_llr=None, repeat=False, small=False):
    """k = 1024: the radix select with s_selk full; 1025: the first k on the argmax sweeps; a k above every row's candidates: the `wk == 0` break, emitted < k.
    small: the same construction on a B 400 columns wide (users of 170 / 12 columns)."""
    mats = dense_problem(400, 170, 12) if small else dense_problem()
    want = dense_classes(mats, k)
    if small:                                         # (400 columns: a table holds the row up to k = 10521)
        assert want == ([0, 0, 1, 2, 0, 0, 0] if k == 1025 else [0, 0, 0, 0, 0, 0, 3]), want
    else:
        assert want == ([0, 0, 0, 0, 0, 1, 2] if k <= 1025 else [0, 0, 0, 0, 0, 0, 3]), want
    _, ref = checked(sess, mats, k, want, min_llr=min_llr, repeat=repeat)
    lens = lens_of(ref[1])
    if k <= 1025 and not small and min_llr is None:
        assert lens.tolist() == [k, k, k], lens       # every row is cut
    if k >= 20000 or small:
        assert lens.max() < k and lens.min() > 0, lens   # no row reaches k: every sweep loop ends at the break
    return lens


def case_self_pair(sess, k=1025, repeat=False):
    """B'B of dense_problem's B alone, items [0, 3): exclude_self inside the dense global kernel."""
    b = dense_problem()[1]
    lens_b = np.diff(b.row_ptr)
    cp, ri = O.transpose(b)
    want = [0] * 7
    for i in range(3):
        holders = ri[cp[i]:cp[i + 1]]
        want[class_of(int(lens_b[holders].sum()), holders.size, b.n_cols, k)] += 1
    assert want == [0, 0, 0, 0, 0, 0, 3], want
    hosts, ref = checked(sess, [b], k, want, item_hi=3, repeat=repeat)
    rp, ci, _ = hosts[0]
    assert lens_of(ref[0]).tolist() == [k, k, k]
    assert not np.any(ci == np.repeat(np.arange(3), np.diff(rp))), "self pair in B'B"


def case_sweep_ties(sess, k=1025, n_cols=65_537, n_tied=11_000, repeat=False):
    """column_digit_ties_case's construction at k = 1025: 11 000 candidates of exactly equal LLR, so the argmax sweeps cut -- and order -- the row by
    column ascending alone.  Exact ids."""
    cols = logic.tied_columns(n_cols, n_tied)
    assert cols.size > 10 * k and cols.max() < n_cols
    holders, n_users = 2, 42
    a = logic.csr_from_pairs(n_users, 2, np.arange(holders + 10), np.concatenate([np.zeros(holders, np.int64), np.ones(10, np.int64)]))
    b = logic.csr_from_pairs(n_users, n_cols, np.repeat(np.arange(holders), cols.size), np.tile(cols, holders))
    assert class_of(holders * cols.size, holders, n_cols, k) == DENSE
    hosts, ref = checked(sess, [a, b], k, one_row(DENSE), exact_ids=True, repeat=repeat)
    rp, ci, llr = hosts[1]
    assert rp[1] == k and np.array_equal(ci[:k], np.sort(cols)[:k]) and np.unique(llr[:k]).size == 1   # (what exact ids against the oracle already say)


def case_context(lib, device, k, flags, repeat=False):
    """dense_problem through Context + cross_occurrence_context: the context's output sizing, compact_indicators for rows far beyond a wave and -- with
    URCCO_FLAG_UNORDERED_ROWS, rows compared through sort_rows -- the unordered store branch of the dense global kernel."""
    from universal_recommender_amd.device import Context, cross_occurrence_context
    mats = dense_problem()
    params = [P(k), P(k)]
    want = dense_classes(mats, k)
    assert want[DENSE] >= 2
    ref = O.cross_occurrence_downsampled(mats, params, 5)
    canon = sort_rows if flags & _lib.FLAG_UNORDERED_ROWS else (lambda got: got)
    ctx = Context(device, lib, flags=flags)
    try:
        runs = []
        for _ in range(2 if repeat else 1):
            out = cross_occurrence_context(ctx, [to_dev(m, device) for m in mats], to_params(params), 5)
            runs.append([(canon(o.to_host()), o.stats.cpu().numpy().copy()) for o in out])      # (a context reuses its output pool)
        for (got, st), r in zip(runs[0], ref):
            assert int(st[0]) == r.pairs, f"pairs {int(st[0])} vs oracle {r.pairs}"
            assert int(st[1 + 4 * 7]) == 0, "LDS accumulator overflow reported"
            check_indicators(got, r)
        rows = runs[0][1][1][1:8].tolist()
        assert rows == want, (k, rows, want)
        assert lens_of(ref[1]).tolist() == [k, k, k]
        for d, (x, y) in enumerate(zip(runs[0], runs[-1])):
            assert_same_bytes(x[0], y[0], f"event {d}")
    finally:
        ctx.close()


# ---- the parameter lists of the two drivers ---------------------------------------------------------------------------------------------------------
EDGES = [(E, family, which) for E in TABLE_WORDS for family in ("hashed", "column")
         for which in ("edge", "edge_k-1", "above", "uncut") + (("edge_no_prefilter",) if family == "hashed" else ())]
SLOW_ON_THE_SIMULATOR = [(32768, "hashed", "above"), (32768, "column", "above")]      # 5460 argmax sweeps
EDGE_ID = "{}-{}-{}".format


def mixed_id(c):
    return f"{c[0]}x{c[2]}of{c[1]}-k{c[3]}"
