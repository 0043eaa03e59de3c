"""The boundary check of the host level (validate_csr_kernel, csrc/cco_misc.hip, launched per shard from urcco_context_stage) at the geometries a 4-entry
matrix never reaches, shared by test_sim_boundary_check.py and test_gpu_boundary_check.py.  Everything goes through the host level as the Scala host
calls it (SimilarityAnalysis.cooccurrencesIDSs -> urcco_cross_occurrence_downsampled): a rejected build raises UrccoError(BAD_ARG) whose message
carries the dataset index and the EXACT number of violations -- one per bad entry, one per bad row_ptr row, `violations` below restates the rule --
and after every rejection a build of the untouched matrices on the same library equals the C oracle.

Geometry: G = 2^clamp(ceil_log2(ceil(nnz / n_rows)), 1, 6) lanes walk a row, 256 / G rows per block, min(ceil(n_rows / (256 / G)), 16 CUs) blocks.  Three
base matrices (average row length ~1.5, ~5.5, ~40: G = 2, 8, 64), each with rows of 2 G + 3 entries at four places: the first row, the last row, a row
in the last block of the first grid round and a row in the second grid round -- the row count follows from the CU count of the device under test."""
import re

import numpy as np
import pytest

from helpers import check_indicators
from oracle import c_oracle as O
from universal_recommender_amd import _lib
from universal_recommender_amd import similarity_analysis as SA
from universal_recommender_amd.indexed_dataset import BiDictionary, IndexedDataset

N_COLS = 500
K, MAX_ROWS, SEED = 10, 30, 99
PLACES = ("first row", "last row", "last block of the first round", "second round")
KINDS = ("decreasing", "duplicate")
INT32_MAX = 2 ** 31 - 1
# row lengths are drawn from [lo, hi), per G
ROW_LENGTHS = {2: (0, 4), 8: (3, 9), 64: (30, 50)}


def lanes_per_row(nnz, n_rows):
    avg = -(-nnz // n_rows)
    g_log2 = min(max((avg - 1).bit_length(), 1), 6)
    return 1 << g_log2


def violations(row_ptr, col_idx, n_cols):
    """What the check counts, written out plainly: a row whose [start, end) runs backwards or is not inside [0, nnz] counts once and none of its
    entries is looked at; in every other row each entry that is outside [0, n_cols) or not above its predecessor IN THE ROW counts once."""
    rp, ci = np.asarray(row_ptr, np.int64), np.asarray(col_idx, np.int64)
    s, e = rp[:-1], rp[1:]
    bad_row = (s < 0) | (e < s) | (e > rp[-1])
    s, n = s[~bad_row], (e - s)[~bad_row]
    p = np.repeat(s, n) + np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)      # the entries of the walkable rows (rows may overlap)
    first = p == np.repeat(s, n)
    j, before = ci[p], ci[np.maximum(p - 1, 0)]
    return int(bad_row.sum()) + int(((j < 0) | (j >= n_cols) | (~first & (before >= j))).sum())


class Base:
    """One valid matrix of a chosen G, its long rows, and (lazily, once) the oracle's indicators of a build of it alone."""

    def __init__(self, G, n_cu, seed=0):
        rng = np.random.default_rng(100 + G + seed)
        self.G, self.L = G, 2 * G + 3
        gpb = 256 // G
        self.round_rows = 16 * n_cu * gpb                       # rows of one round of the full grid
        n_rows = self.round_rows + gpb + 3                      # a second round of a little more than one block
        lo, hi = ROW_LENGTHS[G]
        lens = rng.integers(lo, hi, n_rows)
        self.rows = {"first row": 0, "last row": n_rows - 1, "last block of the first round": self.round_rows - gpb // 2 - 1,
                     "second round": self.round_rows + gpb // 2}
        for r in self.rows.values():
            lens[r] = self.L
        rp = np.zeros(n_rows + 1, np.int64)
        np.cumsum(lens, out=rp[1:])
        # every row: first column and gaps drawn from [1, N_COLS / longest row], summed up inside the row -- ascending, distinct, below N_COLS
        step = rng.integers(1, N_COLS // max(self.L, hi) + 1, int(rp[-1]))
        run = np.concatenate([[0], np.cumsum(step)])
        ci = (run[1:] - np.repeat(run[rp[:-1]], lens) - 1).astype(np.int32)
        assert ci.min() >= 0 and ci.max() < N_COLS, (ci.min(), ci.max())
        self.m = O.Csr(n_rows, N_COLS, rp, ci)
        grid = min(-(-n_rows // gpb), 16 * n_cu)
        assert lanes_per_row(self.m.nnz, n_rows) == G, (self.m.nnz, n_rows)
        assert grid == 16 * n_cu and self.rows["second round"] >= grid * gpb > self.rows["last block of the first round"] >= (grid - 1) * gpb
        assert violations(rp, ci, N_COLS) == 0
        self.users = BiDictionary([f"u{i}" for i in range(n_rows)])
        self.items = BiDictionary([f"i{i}" for i in range(N_COLS)])
        self._ref = None

    def ids(self, row_ptr=None, col_idx=None, n_cols_items=None):
        return IndexedDataset(self.m.row_ptr if row_ptr is None else row_ptr, self.m.col_idx if col_idx is None else col_idx, self.users,
                              n_cols_items or self.items)

    def offsets(self):
        return offsets(self.G)

    def planted(self, plants):
        """A copy of col_idx with the given (place, entry offset t, kind) planted in order; kind also: an int = that value written at t."""
        ci = self.m.col_idx.copy()
        for place, t, kind in plants:
            s = int(self.m.row_ptr[self.rows[place]])
            assert 1 <= t < self.L or (t == 0 and not isinstance(kind, str))
            if kind == "decreasing":
                ci[s + t - 1], ci[s + t] = ci[s + t], ci[s + t - 1]
            elif kind == "duplicate":
                ci[s + t] = ci[s + t - 1]
            else:
                ci[s + t] = kind
        return ci

    def check_good_build(self, lib):
        if self._ref is None:
            self._ref = O.cross_occurrence_downsampled([self.m], [O.DatasetParams(MAX_ROWS, K, None)], SEED)
        res = SA.cooccurrencesIDSs([self.ids()], randomSeed=SEED, maxInterestingItemsPerThing=K, maxNumInteractions=MAX_ROWS, library=lib)
        check_indicators((res[0].row_ptr, res[0].col_idx, res[0].values), self._ref[0])


_bases = {}


def base(G, n_cu):
    if (G, n_cu) not in _bases:
        _bases[(G, n_cu)] = Base(G, n_cu)
    return _bases[(G, n_cu)]


def expect_rejection(lib, datasets, dataset, count):
    with pytest.raises(_lib.UrccoError) as ei:
        SA.cooccurrencesIDSs(datasets, randomSeed=SEED, maxInterestingItemsPerThing=K, maxNumInteractions=MAX_ROWS, library=lib)
    assert ei.value.status == _lib.BAD_ARG, ei.value
    m = re.search(r"dataset (\d+): (\d+) invalid entries", str(ei.value))
    assert m, str(ei.value)
    print(f"reported: dataset {m.group(1)}, {m.group(2)} invalid entries; planted: dataset {dataset}, {count}")
    assert (int(m.group(1)), int(m.group(2))) == (dataset, count), str(ei.value)


def rejected_then_good(lib, b, col_idx=None, row_ptr=None, count=None):
    """One rejected build of b's matrix with col_idx / row_ptr replaced (count: violations planted, checked against `violations`), then the untouched one."""
    rp = b.m.row_ptr if row_ptr is None else row_ptr
    ci = b.m.col_idx if col_idx is None else col_idx
    want = violations(rp, ci, N_COLS)
    assert want > 0 and (count is None or want == count), (want, count)
    expect_rejection(lib, [b.ids(rp, ci)], 0, want)
    b.check_good_build(lib)
    return want


# ---- in-range violations (simulator and hardware) --------------------------------------------------------------------------------------------------------
def offsets(G):
    """Entry offsets inside a long row (L = 2 G + 3 entries): 1, G - 1, G, G + 1, 2 G, L - 1 -- the second entry, both sides of a lane group's first
    lane (its predecessor belongs to the previous group's last lane) in the first and the second sweep, the row's last entry."""
    return sorted({1, G - 1, G, G + 1, 2 * G, 2 * G + 2})


def case_in_range(lib, n_cu, G, kind, place, t):
    """Entries t - 1 and t swapped (decreasing) or entry t - 1 copied into entry t (duplicate): exactly one violation."""
    b = base(G, n_cu)
    rejected_then_good(lib, b, col_idx=b.planted([(place, t, kind)]), count=1)


def case_all_at_once(lib, n_cu, G):
    b = base(G, n_cu)
    plants = []
    for i, place in enumerate(PLACES):
        if i % 2 == 0:                                            # duplicates at every offset (ascending: each copies what the one before left)
            plants += [(place, t, "duplicate") for t in b.offsets()]
        else:                                                     # swaps at offsets two apart at least (a swap touches t - 1 and t)
            last = -2
            for t in b.offsets():
                if t - last >= 2:
                    plants.append((place, t, "decreasing"))
                    last = t
    rejected_then_good(lib, b, col_idx=b.planted(plants), count=len(plants))
    return len(plants)


def case_secondary(lib, n_cu, bad_dataset):
    """Three event types; the violation sits in dataset 1 or 2: the message names it, and the process-wide context -- whose primary chain had already
    started -- builds the untouched three afterwards."""
    b = base(8, n_cu)
    mats = [b.m] + [O.Csr(b.m.n_rows, N_COLS + d, b.m.row_ptr, b.m.col_idx + d) for d in (1, 2)]   # the same rows over wider item dictionaries, shifted
    items = [b.items] + [BiDictionary([f"j{d}_{i}" for i in range(N_COLS + d)]) for d in (1, 2)]
    good = [IndexedDataset(m.row_ptr, m.col_idx, b.users, it) for m, it in zip(mats, items)]
    bad_ci = mats[bad_dataset].col_idx.copy()
    s = int(b.m.row_ptr[b.rows["second round"]])
    bad_ci[s + b.G] = bad_ci[s + b.G - 1]
    bad = list(good)
    bad[bad_dataset] = IndexedDataset(mats[bad_dataset].row_ptr, bad_ci, b.users, items[bad_dataset])
    ref = O.cross_occurrence_downsampled(mats, [O.DatasetParams(MAX_ROWS, K, None)] * 3, SEED)
    expect_rejection(lib, bad, bad_dataset, 1)
    res = SA.cooccurrencesIDSs(good, randomSeed=SEED, maxInterestingItemsPerThing=K, maxNumInteractions=MAX_ROWS, library=lib)
    for r, o in zip(res, ref):
        check_indicators((r.row_ptr, r.col_idx, r.values), o)


def case_first_column_below_previous_last(lib, G=2):
    """The false-positive control (the `p > s` guard): a VALID matrix in which every row starts with a column below the previous row's last one and row 0
    starts with column 0 must build and equal the oracle.  (With a guard page before every buffer a read of col_idx[-1] faults.)"""
    rng = np.random.default_rng(3)
    n_rows = 1000
    lens = np.full(n_rows, 2) if G == 2 else rng.integers(5, 9, n_rows)
    rp = np.zeros(n_rows + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    ci = np.empty(int(rp[-1]), np.int32)
    for r in range(n_rows):                                       # column 0 or 1 first (row 0: column 0), then columns from the upper half
        row = np.sort(rng.choice(np.arange(N_COLS // 2, N_COLS), lens[r] - 1, replace=False))
        ci[rp[r]:rp[r + 1]] = np.concatenate([[0 if r == 0 else r % 2], row])
    assert ci[0] == 0 and np.all(ci[rp[1:-1]] < ci[rp[1:-1] - 1]) and violations(rp, ci, N_COLS) == 0
    assert lanes_per_row(int(rp[-1]), n_rows) == G
    m = O.Csr(n_rows, N_COLS, rp, ci)
    ids = IndexedDataset(rp, ci, BiDictionary([f"u{i}" for i in range(n_rows)]), BiDictionary([f"i{i}" for i in range(N_COLS)]))
    ref = O.cross_occurrence_downsampled([m], [O.DatasetParams(MAX_ROWS, K, None)], SEED)
    res = SA.cooccurrencesIDSs([ids], randomSeed=SEED, maxInterestingItemsPerThing=K, maxNumInteractions=MAX_ROWS, library=lib)
    check_indicators((res[0].row_ptr, res[0].col_idx, res[0].values), ref[0])


# ---- out-of-range columns and row_ptr violations (simulator only: a hole here would send the build behind it out of bounds) -----------------------------
OUT_OF_RANGE = {"n_cols": N_COLS, "minus one": -1, "INT32_MAX": INT32_MAX}


def case_out_of_range(lib, n_cu, G, what, place):
    """Column = n_cols, -1 or INT32_MAX at every offset (t = 0 included).  A too large column also makes its successor `not above its predecessor`:
    2 violations, except for the row's last entry; -1: one.  The build of the untouched matrix follows the seven rejections of one (G, value, place),
    not each of them: a simulated build costs 70 ms whatever its size, and there are 252 of these rejections."""
    b = base(G, n_cu)
    for t in [0] + b.offsets():
        ci = b.planted([(place, t, OUT_OF_RANGE[what])])
        want = 1 if what == "minus one" or t == b.L - 1 else 2
        assert violations(b.m.row_ptr, ci, N_COLS) == want
        expect_rejection(lib, [b.ids(col_idx=ci)], 0, want)
    b.check_good_build(lib)


def case_row_ptr(lib, n_cu, G, what):
    """An interior row_ptr[r] of a long row in the second round: lowered below row_ptr[r - 1]; raised above nnz (row r - 1 and row r count once each and
    none of their entries is read: the walk would leave col_idx); raised a little, so that row_ptr decreases to row_ptr[r + 1] and is back in order there."""
    b = base(G, n_cu)
    r = b.rows["second round"]
    rp = b.m.row_ptr.copy()
    if what == "lowered":
        rp[r] = rp[r - 2] - 1 if rp[r - 2] > 0 else 0
        assert rp[r] < rp[r - 1]
    elif what == "above nnz":
        rp[r] = rp[-1] + 100_000
    else:
        rp[r] = rp[r + 1] + 2                                     # row r - 1 swallows row r and two entries of row r + 1; row r runs backwards
        assert rp[r] <= rp[-1]
    want = rejected_then_good(lib, b, row_ptr=rp)
    if what == "above nnz":
        assert want == 2
    return want


# ---- shards: rp0 != 0 (simulator: several simulated devices on a caller-made context; the library cuts the users itself) ---------------------------------
def shard_cuts(row_ptr, n_shards):
    """urcco_context_stage's user ranges, written out again: cut g = the first user, not before cut g - 1, at which the interactions so far reach
    floor(total / n_shards) g."""
    cuts = [0]
    for g in range(1, n_shards):
        cuts.append(max(cuts[-1], int(np.searchsorted(row_ptr, int(row_ptr[-1]) // n_shards * g, side="left"))))
    return cuts + [len(row_ptr) - 1]


class ShardBase:
    """A valid matrix of the chosen G (inside every shard) whose SECOND shard begins and ends with a row of 2 G + 3 entries."""

    def __init__(self, G, n_shards, n_rows=3001):
        rng = np.random.default_rng(G + n_shards)
        self.G, self.L = G, 2 * G + 3
        lo, hi = ROW_LENGTHS[G]
        base_lens = rng.integers(lo, hi, n_rows)
        long_rows = ()
        for _ in range(20):                                       # the long rows move the cuts: repeat until they sit on the cuts they make
            lens = base_lens.copy()
            lens[list(long_rows)] = self.L
            rp = np.zeros(n_rows + 1, np.int64)
            np.cumsum(lens, out=rp[1:])
            cuts = shard_cuts(rp, n_shards)
            if long_rows == (cuts[1], cuts[2] - 1):
                break
            long_rows = (cuts[1], cuts[2] - 1)
        else:
            raise AssertionError("the cuts do not settle")
        self.cuts, self.rows = cuts, {"first row of the second shard": cuts[1], "last row of the second shard": cuts[2] - 1}
        assert 0 < cuts[1] < cuts[2] - 1 and rp[cuts[1]] > 0
        step = rng.integers(1, N_COLS // max(self.L, hi) + 1, int(rp[-1]))
        run = np.concatenate([[0], np.cumsum(step)])
        ci = (run[1:] - np.repeat(run[rp[:-1]], lens) - 1).astype(np.int32)
        assert violations(rp, ci, N_COLS) == 0
        for a, b in zip(cuts, cuts[1:]):
            assert lanes_per_row(int(rp[b] - rp[a]), b - a) == G
        self.m = O.Csr(n_rows, N_COLS, rp, ci)
        self.ref = O.cross_occurrence_downsampled([self.m], [O.DatasetParams(MAX_ROWS, K, None)], SEED)

    planted = Base.planted

    def build(self, lib, ctx, col_idx):
        """urcco_context_cross_occurrence (host arrays in, host indicators out) on the caller's context."""
        import ctypes as C
        ci = np.ascontiguousarray(col_idx, np.int32)
        arr = (_lib.Dataset * 1)()
        arr[0].matrix.n_rows, arr[0].matrix.n_cols = self.m.n_rows, N_COLS
        arr[0].matrix.row_ptr, arr[0].matrix.col_idx = self.m.row_ptr.ctypes.data, ci.ctypes.data
        arr[0].max_elements_per_row, arr[0].max_interesting_elements, arr[0].has_min_llr = MAX_ROWS, K, 0
        out, stats = (_lib.Indicators * 1)(), (_lib.DatasetStats * 1)()
        try:
            _lib.check(lib.urcco_context_cross_occurrence(ctx.handle, arr, 1, SEED, out, stats), lib)
            o, nnz = out[0], int(out[0].nnz)
            return (np.ctypeslib.as_array(o.row_ptr, shape=(o.n_rows + 1,)).copy(), np.ctypeslib.as_array(o.col_idx, shape=(max(nnz, 1),))[:nnz].copy(),
                    np.ctypeslib.as_array(o.llr, shape=(max(nnz, 1),))[:nnz].copy())
        finally:
            lib.urcco_free_indicators(out, 1)


_shard_bases = {}


def case_shard(lib, ctx, n_shards, G, kind, place):
    """Every offset in the first / the last row of the second shard (whose row_ptr slice starts at rp0 > 0): one violation each, then the untouched build."""
    if (G, n_shards) not in _shard_bases:
        _shard_bases[(G, n_shards)] = ShardBase(G, n_shards)
    b = _shard_bases[(G, n_shards)]
    for t in offsets(G):
        ci = b.planted([(place, t, kind)])
        assert violations(b.m.row_ptr, ci, N_COLS) == 1
        with pytest.raises(_lib.UrccoError) as ei:
            b.build(lib, ctx, ci)
        m = re.search(r"dataset (\d+): (\d+) invalid entries", str(ei.value))
        assert ei.value.status == _lib.BAD_ARG and m and (int(m.group(1)), int(m.group(2))) == (0, 1), (t, str(ei.value))
        check_indicators(b.build(lib, ctx, b.m.col_idx), b.ref[0])
