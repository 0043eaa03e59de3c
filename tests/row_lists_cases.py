"""One build that populates EVERY row list of the binning pass (csrc/cco_kernels.h, RowList; csrc/cco_rows.hip, internal_bin), shared by
test_sim_row_lists.py and test_gpu_row_lists.py.  The other case files fill a few lists at a time, and a launch whose run of lists ends one list too far
produces identical outputs -- the rows are merely computed twice.  Here, with the classes split (URCCO_MICRO_SPLIT_ROWS=0 as the tests run, k = 10), every one
of the 13 lists holds at least two rows, empty item rows lie before, between and behind them, and the build is checked against the oracle, bit for bit
against the same build with the small-row bodies off (NO_SMALL_WAVE | NO_BLOCK_SMALL_WAVE) and in the plain form (UNPACKED_COUNTS: one launch per bin), the
rows per public bin against choose_bin's model, and -- what fails when any row is run twice or not at all -- the distinct-candidate word of the statistics
(stats[2 + 4 * NBINS] while stage timing is on) against the numpy count of distinct (row, column) pairs, in each of the three builds."""
import numpy as np

from block_small_wave_cases import build, spread
from direct_rank_cases import class_of
from helpers import compare_with_oracle
from oracle import c_oracle as O
from prefilter_cases import assert_bit_equal
from small_wave_cases import P, distinct, repeated, rows_of_build
from universal_recommender_amd import _lib

K, SEED, NBINS = 10, 3, 7
LISTS = ["micro <= 16", "micro <= 32", "micro", "one-wave <= 128 pairs", "one-wave <= 256 pairs", "one-wave <= 128 users", "one-wave", "small-block <= 128 users",
         "small-block", "block", "half-CU", "CU", "multi-pass"]
BODIES_OFF = _lib.DBG_NO_SMALL_WAVE | _lib.DBG_NO_BLOCK_SMALL_WAVE


def list_of(w, ca, n_cols, k):
    """internal_bin of cco_rows.hip with the classes split: the index of the row's list in LISTS."""
    c = class_of(w, ca, n_cols, k)
    if c == 0:
        return 0 if (w <= 16 and ca <= 16) else (1 if (w <= 32 and ca <= 32) else 2)
    if c == 1:
        return 6 if ca > 128 else (5 if (ca > 64 or w > 256) else (3 if w <= 128 else 4))
    if c == 2:
        return 7 if (ca <= 128 and w <= 512) else 8
    return c + 6


def workload():
    """[A, B]: at k = 10 a table of E words holds a row of (E - 32) / 3 pairs -- 330, 1354, 2720, 5450, 10912 -- so the heavy classes start at 1355, 2721 and
    5451 pairs, and the multi-pass class at 10913 pairs once B has as many columns (the two all-distinct CU rows alone bring them).  Rows at both edges of
    every list, all-distinct columns and heavily repeated ones; three item rows without a user."""
    specs = [distinct(5), repeated(16, 16), distinct(17), repeated(32, 32), distinct(64), spread(40, 64, 30),                    # the micro class's lists
             distinct(65), spread(128, 64, 40), distinct(129), repeated(256), distinct(257), spread(100, 65, 40), spread(330, 128, 128),
             spread(100, 129, 40), spread(330, 200, 150),                                                                        # ... the one-wave class's
             distinct(331), spread(512, 128, 100), distinct(513), spread(400, 129, 60), distinct(1354),                          # the small-block class's
             distinct(1355), repeated(2720, 80), distinct(2721), repeated(5450, 50),                                             # block, half-CU
             distinct(5451), distinct(5500), repeated(10912, 64), repeated(10913, 107), distinct(10913)]                         # CU, multi-pass
    (a, b), _ = build(specs)
    ids = np.arange(len(specs)) + 1 + (np.arange(len(specs)) >= 10)      # item rows 0, 11 and the last one stay empty
    return [O.Csr(a.n_rows, len(specs) + 3, a.row_ptr, ids[a.col_idx].astype(np.int32)), b]


def case_every_list(sess):
    mats, params = workload(), [P(K), P(K)]
    rows = rows_of_build(mats, params, SEED)      # (cA, k11[D], cB[D]) of every non-empty row of A'A and of A'B
    want_bins = [np.bincount([class_of(int(k11.sum()), ca, m.n_cols, K) for ca, k11, _ in r], minlength=NBINS) for r, m in zip(rows, mats)]
    want_distinct = [sum(k11.size for _, k11, _ in r) for r in rows]
    per_list = np.bincount([list_of(int(k11.sum()), ca, mats[1].n_cols, K) for ca, k11, _ in rows[1]], minlength=len(LISTS))
    assert per_list.min() >= 2 and mats[0].n_cols - len(rows[1]) == 3, dict(zip(LISTS, per_list.tolist()))
    outs = {}
    sess.set_timing(True)
    try:
        for name, bits in (("default", 0), ("bodies off", BODIES_OFF), ("plain form", _lib.DBG_UNPACKED_COUNTS)):
            sess.set_debug(bits)
            outs[name], _, stats = compare_with_oracle(sess, mats, params, SEED)
            got_bins = [s[0][1:1 + NBINS].tolist() for s in stats]
            got_distinct = [int(s[0][2 + 4 * NBINS]) for s in stats]
            print(f"{name}: rows per bin {got_bins}, distinct candidates {got_distinct} (numpy: {want_distinct}); rows per list of A'B {per_list.tolist()}")
            assert got_bins == [w.tolist() for w in want_bins], (name, got_bins, want_bins)
            assert got_distinct == want_distinct, (name, got_distinct, want_distinct)
    finally:
        sess.set_debug(0)
        sess.set_timing(False)
    assert_bit_equal(outs["default"], outs["bodies off"])
    assert_bit_equal(outs["default"], outs["plain form"])
