"""Kernel LOGIC on CPU: the unchanged HIP sources compiled against tests/hostsim and compared with the oracle.
These are not parity claims (those are the -m gpu tests); they catch indexing / hashing / compaction / selection
bugs before a GPU slot is spent, and they cover the C-ABI orchestration (scratch arena, stage order)."""
import numpy as np
import pytest
import torch

from helpers import compare_with_oracle, guarded, rand_csr, to_dev
from oracle import c_oracle as O
from universal_recommender_amd import _lib


def P(max_rows=500, k=50, min_llr=None):
    return O.DatasetParams(max_rows, k, min_llr)


def test_small_three_events_all_modes(sim_session):
    rng = np.random.default_rng(1)
    mats = [rand_csr(rng, 300, 80, 6), rand_csr(rng, 300, 40, 9), rand_csr(rng, 300, 7, 2)]
    compare_with_oracle(sim_session, mats, [P(), P(), P()], 42)
    compare_with_oracle(sim_session, mats, [P(20, 5), P(30, 7, 0.5), P(500, 3)], 7)
    compare_with_oracle(sim_session, mats, [P(4, 5), P(6, 7), P(2, 3)], 7, mode=1)
    compare_with_oracle(sim_session, mats, [P(4, 5), P(6, 7), P(2, 3)], -3, mode=0)


def test_hash_tables_and_all_bins(sim_session):
    """Enough columns that no table covers B (hash mode), rows spread over the wave / block / CU accumulators."""
    rng = np.random.default_rng(2)
    a = rand_csr(rng, 4000, 20000, 12, zipf_s=1.2)
    b = rand_csr(rng, 4000, 30000, 25, zipf_s=1.1)
    _, _, stats = compare_with_oracle(sim_session, [a, b], [P(10000, 50), P(10000, 20)], 5)
    bins = stats[1][0][1:8]          # micro, wave, small block, block, half CU, CU, global
    assert bins[1] > 0 and bins[2] + bins[3] > 0 and bins[4] + bins[5] > 0, bins


def _micro_case(rng, n_items_a, users_per_item, b_cols, b_len_lo, b_len_hi, empty_frac=0.2):
    """A: every item held by `users_per_item`-ish users who hold nothing else; B: rows of b_len_lo..b_len_hi columns (some empty), so an
    item's cooccurrence pairs -- and, with many columns, its distinct candidates -- land anywhere in 1..64."""
    upi = rng.integers(1, users_per_item + 1, n_items_a)
    n_users = int(upi.sum()) + 5                       # a few users without a primary event
    a_cols = np.repeat(np.arange(n_items_a, dtype=np.int32), upi)
    a_rp = np.concatenate([np.arange(a_cols.size + 1, dtype=np.int64), np.full(5, a_cols.size, np.int64)])
    a = O.Csr(n_users, n_items_a, a_rp, a_cols)
    lens = rng.integers(b_len_lo, b_len_hi + 1, n_users)
    lens[rng.random(n_users) < empty_frac] = 0
    rows = [np.sort(rng.choice(b_cols, size=min(int(l), b_cols), replace=False)).astype(np.int32) for l in lens]
    b_rp = np.zeros(n_users + 1, np.int64)
    np.cumsum([r.size for r in rows], out=b_rp[1:])
    return a, O.Csr(n_users, b_cols, b_rp, np.concatenate(rows) if rows else np.zeros(0, np.int32))


def test_micro_class_every_ranking_form(sim_session):
    """Rows of the micro class (<= 64 users and pairs) with 1..64 distinct candidates: the candidate's owner is the lane that claimed its
    column, rows of <= 16 / <= 32 / <= 64 candidates are ranked by four / two / one replica(s), k cuts inside the row, columns repeat
    (k11 > 1) and LLRs tie (few columns), empty B' rows sit before, between and behind the users of a row."""
    rng = np.random.default_rng(77)
    for b_cols, lo, hi, upi, k in [(5000, 1, 16, 4, 50), (5000, 8, 32, 2, 50), (5000, 20, 60, 1, 50), (5000, 1, 30, 3, 7), (40, 1, 12, 5, 50),
                                   (40, 1, 12, 5, 3), (200, 0, 3, 20, 50), (300, 30, 64, 1, 64)]:
        a, b = _micro_case(rng, 400, upi, b_cols, lo, hi)
        _, _, stats = compare_with_oracle(sim_session, [a, b], [P(100000, k), P(100000, k)], 13)
        assert stats[1][0][1] > 100, stats[1][0][1:8]   # rows of the micro class in A'B


def micro_sub_range_rows(a, b, item_lo=0, item_hi=None):
    """Plain numpy reference of the micro class's three size ranges for the item rows [item_lo, item_hi) of A'B, from the DOWN-SAMPLED
    matrices: w[i] = sum over the users u of column i of A' of len(B' row u) (the row's pairs), cA[i] = users of column i; the class holds
    the rows with 0 < w <= 64 and 0 < cA <= 64 (choose_bin, csrc/cco_rows.hip; a cA of <= 64 fits the packed count of every catalogue width).
    Returns the rows with (w <= 16 and cA <= 16, the rest with w <= 32 and cA <= 32, the rest): with the class split, the first two are the
    shared-wave sub-lists -- stats[STATS_LEN - 1] is their sum; unsplit, all three are the one list and the word is 0."""
    item_hi = a.n_cols if item_hi is None else item_hi
    users = np.repeat(np.arange(a.n_rows, dtype=np.int64), np.diff(a.row_ptr))
    cols = a.col_idx[:a.nnz]
    w = np.bincount(cols, weights=np.diff(b.row_ptr)[users].astype(np.float64), minlength=a.n_cols).astype(np.int64)   # (exact: far below 2^53)
    ca = np.bincount(cols, minlength=a.n_cols)
    w, ca = w[item_lo:item_hi], ca[item_lo:item_hi]
    micro = (w > 0) & (ca > 0) & (w <= 64) & (ca <= 64)
    s16 = micro & (w <= 16) & (ca <= 16)
    s32 = micro & ~s16 & (w <= 32) & (ca <= 32)
    return int(s16.sum()), int(s32.sum()), int((micro & ~s16 & ~s32).sum())


def micro_sub_range_rows_of_build(mats, params, seed, mode=0, item_lo=0, item_hi=None):
    """micro_sub_range_rows of every event type of a build, the matrices down-sampled by the oracle."""
    ds = [O.downsample(m, O.column_counts(m), seed, p.max_elements_per_row, mode) for m, p in zip(mats, params)]
    return [micro_sub_range_rows(ds[0], b, item_lo, item_hi) for b in ds]


def test_stats_word_31_counts_the_shared_wave_rows(sim_session):
    """stats[STATS_LEN - 1] = rows binned into the two shared-wave sub-lists of the first accumulator class (the word by which the GPU tests tell which
    form of that class a build ran): exact against micro_sub_range_rows for every event type, on the builds of
    test_micro_class_every_ranking_form and on a rand_csr build, whole and as an item range.  Both workloads hold rows in all three size
    ranges, so a word that counted the wrong sub-lists (the <= 64 remainder too, only the first) differs.  The pytest process sets the
    threshold of the split to 0 (conftest.py); under another value the word must be 0 for builds below it."""
    import os
    min_rows = int(os.environ.get("URCCO_MICRO_SPLIT_ROWS") or 1000000)

    def check(mats, params, seed, item_lo=0, item_hi=None):
        _, _, stats = compare_with_oracle(sim_session, mats, params, seed, 0, item_lo, item_hi)
        ref = micro_sub_range_rows_of_build(mats, params, seed, 0, item_lo, item_hi)
        n = (mats[0].n_cols if item_hi is None else item_hi) - item_lo
        for (st, _, _), (r16, r32, r64) in zip(stats, ref):
            assert int(st[1]) == r16 + r32 + r64, (st[1:8], r16, r32, r64)          # the reference's class membership is the library's
            assert int(st[_lib.STATS_LEN - 1]) == (r16 + r32 if n >= min_rows else 0), (int(st[_lib.STATS_LEN - 1]), r16, r32, r64)
        return np.array(ref)

    rng = np.random.default_rng(77)
    tot = np.zeros((2, 3), np.int64)
    for b_cols, lo, hi, upi, k in [(5000, 1, 16, 4, 50), (5000, 8, 32, 2, 50), (5000, 20, 60, 1, 50), (5000, 1, 30, 3, 7), (40, 1, 12, 5, 50),
                                   (40, 1, 12, 5, 3), (200, 0, 3, 20, 50), (300, 30, 64, 1, 64)]:
        a, b = _micro_case(rng, 400, upi, b_cols, lo, hi)
        tot += check([a, b], [P(100000, k), P(100000, k)], 13)
    assert tot[1].min() > 100 and tot[0][:2].min() > 50, tot     # A'B: all three ranges; A'A (one item per user: w = cA <= 20): the two shared-wave ones
    rng = np.random.default_rng(78)
    mats = [rand_csr(rng, 3000, 2000, 4, zipf_s=0.8), rand_csr(rng, 3000, 500, 5), rand_csr(rng, 3000, 30, 2, empty_frac=0.3)]
    params = [P(100000, 20), P(100000, 20), P(40, 50)]           # (the third event type IS down-sampled: the reference follows the oracle's B')
    ref = check(mats, params, 5)
    assert ref[:2].min() > 50 and ref[2].min() > 0, ref
    part = check(mats, params, 5, 301, 1777)
    assert part[:2].min() > 25 and np.all(part.sum(1) < ref.sum(1)), (part, ref)


def test_global_accumulator_rows(sim_session):
    """Rows that cannot be bounded below an LDS table (w > 10240 with > 16384 columns) take the dense global path."""
    rng = np.random.default_rng(3)
    n_users = 1500
    a = rand_csr(rng, n_users, 40, 6, zipf_s=1.5)
    b = rand_csr(rng, n_users, 17000, 40, zipf_s=0.3)
    _, _, stats = compare_with_oracle(sim_session, [a, b], [P(100000, 10), P(100000, 60)], 11)
    assert stats[1][0][7] > 0, stats[1][0]


def test_packed_count_overflow_goes_global(sim_session):
    """cA[i] larger than the packed count field (many columns -> few count bits) must not use the packed table."""
    rng = np.random.default_rng(4)
    n_users = 3000
    a = rand_csr(rng, n_users, 5, 2, zipf_s=2.0)            # item 0 owned by most users
    b = rand_csr(rng, n_users, 3_000_000, 1.2, zipf_s=0.0)  # 22 key bits -> 10 count bits (max 1023)
    _, _, stats = compare_with_oracle(sim_session, [a, b], [P(1000000, 10), P(1000000, 10)], 3)
    assert stats[1][0][7] > 0


def test_empty_and_ragged_inputs(sim_session):
    rng = np.random.default_rng(5)
    a = rand_csr(rng, 257, 33, 3, empty_frac=0.5)
    b_empty = O.Csr(257, 9, np.zeros(258, np.int64), np.zeros(0, np.int32))
    c = rand_csr(rng, 257, 5000, 1, empty_frac=0.9)
    compare_with_oracle(sim_session, [a, b_empty, c], [P(), P(), P()], 1)
    # primary with no interactions at all
    a0 = O.Csr(10, 4, np.zeros(11, np.int64), np.zeros(0, np.int32))
    compare_with_oracle(sim_session, [a0, rand_csr(rng, 10, 4, 2)], [P(), P()], 1)
    # one user
    compare_with_oracle(sim_session, [rand_csr(rng, 1, 50, 20), rand_csr(rng, 1, 50, 20)], [P(), P()], 1)


def test_item_range_slices_concatenate(sim_session):
    """Disjoint item ranges (the multi-GPU partition) give exactly the rows of the full run."""
    rng = np.random.default_rng(6)
    mats = [rand_csr(rng, 800, 300, 8), rand_csr(rng, 800, 500, 10)]
    ps = [P(40, 10), P(40, 10)]
    full, _, _ = compare_with_oracle(sim_session, mats, ps, 9)
    parts = [compare_with_oracle(sim_session, mats, ps, 9, 0, lo, hi)[0] for lo, hi in [(0, 117), (117, 118), (118, 300)]]
    for d in range(2):
        rp, ci, llr = full[d].to_host()
        cat_ci = np.concatenate([p[d].to_host()[1] for p in parts])
        cat_llr = np.concatenate([p[d].to_host()[2] for p in parts])
        assert np.array_equal(ci, cat_ci) and np.array_equal(llr, cat_llr)


def test_downsample_row_base_matches_sharded_rows(sim_session):
    """sampleDownAndBinarize on a row shard with row_base == the same rows of the unsharded run (RNG keyed by global row)."""
    rng = np.random.default_rng(7)
    m = rand_csr(rng, 1000, 60, 30, zipf_s=1.3)
    dev = sim_session.device
    raw = sim_session.column_counts(guarded(torch.from_numpy(m.col_idx.copy()).to(dev)), m.nnz, m.n_cols)
    full, _ = sim_session.downsample(to_dev(m, dev), m.nnz, raw, 77, 25)
    lo, hi = 333, 901
    shard = O.Csr(hi - lo, m.n_cols, m.row_ptr[lo:hi + 1] - m.row_ptr[lo], m.col_idx[m.row_ptr[lo]:m.row_ptr[hi]])
    part, _ = sim_session.downsample(to_dev(shard, dev), shard.nnz, raw, 77, 25, 0, lo)
    sim_session.synchronize()
    frp, prp = full.row_ptr.cpu().numpy(), part.row_ptr.cpu().numpy()
    fci, pci = full.col_idx.cpu().numpy(), part.col_idx.cpu().numpy()
    assert np.array_equal(frp[lo:hi + 1] - frp[lo], prp)
    assert np.array_equal(fci[frp[lo]:frp[hi]], pci[:prp[-1]])
    ref = O.downsample(m, O.column_counts(m), 77, 25)
    assert np.array_equal(ref.row_ptr, frp) and np.array_equal(ref.col_idx, fci[:frp[-1]])


def test_unaligned_col_idx_takes_scalar_path(sim_session):
    rng = np.random.default_rng(8)
    m = rand_csr(rng, 500, 90, 11)
    dev = sim_session.device
    buf = torch.zeros(m.nnz + 8, dtype=torch.int32, device=dev)
    view = buf[1:1 + m.nnz]                      # 4-byte aligned only
    view.copy_(torch.from_numpy(m.col_idx))
    assert view.data_ptr() % 16 != 0
    cnt = sim_session.column_counts(view, m.nnz, m.n_cols)
    from universal_recommender_amd.device import DevCsr
    out, post = sim_session.downsample(DevCsr(m.n_rows, m.n_cols, guarded(torch.from_numpy(m.row_ptr.copy()).to(dev)), view, m.nnz), m.nnz, cnt, 5, 7)
    sim_session.synchronize()
    assert np.array_equal(cnt.cpu().numpy(), O.column_counts(m))
    ref = O.downsample(m, O.column_counts(m), 5, 7)
    assert np.array_equal(out.row_ptr.cpu().numpy(), ref.row_ptr)
    assert np.array_equal(out.col_idx.cpu().numpy()[:ref.nnz], ref.col_idx)
    assert np.array_equal(post.cpu().numpy()[:m.n_cols], O.column_counts(ref))


def test_downsampling_under_the_32_bit_rng(sim_session):
    """URCCO_RNG_MIX32 (decision D10 b): the same builds with the 32-bit down-sampling RNG OR-ed into the row-rate mode -- device and oracle
    draw the same stream, both row-rate modes, the one-byte threshold prefixes (ties on the prefix fall back to the full 32-bit threshold),
    rows beyond the interaction cap (fractional row rate: their own threshold), a sharded row_base."""
    from oracle import c_oracle
    R = c_oracle.RNG_MIX32
    rng = np.random.default_rng(21)
    a, b, c = rand_csr(rng, 4000, 900, 12, zipf_s=1.1), rand_csr(rng, 4000, 2500, 30), rand_csr(rng, 4000, 12, 3, empty_frac=0.2)
    for mode in (R, R | 1):
        compare_with_oracle(sim_session, [a, b, c], [P(20, 10), P(25, 12), P(500, 50)], 3, mode)
    m = rand_csr(rng, 70000, 90_000, 17, zipf_s=1.0)       # >= 2^20 interactions: the tiled row scan, many thresholds per prefix value
    assert m.nnz >= (1 << 20)
    d = to_dev(m, sim_session.device)
    cnt = sim_session.column_counts(d.col_idx, m.nnz, m.n_cols)
    for mode, base in ((R, 0), (R | 1, 123_456_789)):
        out, post = sim_session.downsample(d, m.nnz, cnt, 11, 9, mode, base)
        sim_session.synchronize()
        ref = O.downsample(m, O.column_counts(m), 11, 9, mode, base)
        ref53 = O.downsample(m, O.column_counts(m), 11, 9, mode & 1, base)
        assert np.array_equal(out.row_ptr.cpu().numpy(), ref.row_ptr) and np.array_equal(out.col_idx.cpu().numpy()[:ref.nnz], ref.col_idx)
        assert np.array_equal(post.cpu().numpy()[:m.n_cols], O.column_counts(ref))
        assert not np.array_equal(ref.row_ptr, ref53.row_ptr)                    # a different stream ...
        assert abs(ref.nnz - ref53.nnz) < 6 * np.sqrt(ref53.nnz)                  # ... that keeps as many interactions


def test_llr_operands_beyond_the_tables(sim_session):
    """The row kernels evaluate a candidate's LLR from five table reads behind ONE range check (llr_candidate, csrc/cco_device.h); operands
    beyond the 4096-entry tables -- a column held by 5000 of 6000 users, no interaction cut -- take the rolled general form (one copy of
    the logarithm).  Both must give the oracle's value: A'A (the hot item's own row: cA beyond the table) and A'B (hot candidates)."""
    rng = np.random.default_rng(33)
    n_users = 6000
    a = rand_csr(rng, n_users, 300, 6, zipf_s=0.7)
    hot = np.sort(rng.choice(n_users, 5000, replace=False))
    b0 = rand_csr(rng, n_users, 200, 4)
    is_hot = np.zeros(n_users, bool)
    is_hot[hot] = True
    rows = [np.unique(np.concatenate([b0.col_idx[b0.row_ptr[u]:b0.row_ptr[u + 1]], [7] if is_hot[u] else []]).astype(np.int32)) for u in range(n_users)]
    rp = np.zeros(n_users + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    b = O.Csr(n_users, 200, rp, np.concatenate(rows))
    assert O.column_counts(b)[7] >= 5000
    _, _, stats = compare_with_oracle(sim_session, [b, a], [P(100000, 50), P(100000, 50)], 9)       # primary = the matrix with the hot column
    _, _, stats = compare_with_oracle(sim_session, [a, b], [P(100000, 50), P(100000, 50)], 9)       # ... and as the secondary


def test_counts_aboard_and_the_count_gather_agree(sim_session):
    """Round 6: B' words carry their column's post-sampling count (urcco_dev_pack_counts) and the row kernels read a candidate's cB off the word
    that claims its accumulator slot -- what every other test of this file runs.  Here (a) the form of rounds 1-5 -- plain column indices, one
    count gather per candidate -- on matrices that fill every accumulator class, and (b) a catalogue of 2^20 columns (11 spare bits in a word)
    with a column held by 3000 users and no interaction cut: that count does not fit, the pack pass says so and the build falls back to the
    gather.  Every row against the oracle in both cases."""
    rng = np.random.default_rng(61)
    a = rand_csr(rng, 3000, 900, 10, zipf_s=1.1)
    b = rand_csr(rng, 3000, 2500, 25, zipf_s=1.0)
    c = rand_csr(rng, 3000, 40, 3)
    sim_session.pack_counts = False
    try:
        compare_with_oracle(sim_session, [a, b, c], [P(200, 20), P(200, 20), P(500, 50)], 17)
    finally:
        sim_session.pack_counts = True
    n_users, n_cols = 4000, 1 << 20
    base = rand_csr(rng, n_users, n_cols, 5)
    hot = np.zeros(n_users, bool)
    hot[rng.choice(n_users, 3000, replace=False)] = True
    rows = [np.unique(np.concatenate([base.col_idx[base.row_ptr[u]:base.row_ptr[u + 1]], [12345] if hot[u] else []]).astype(np.int32)) for u in range(n_users)]
    rp = np.zeros(n_users + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    wide = O.Csr(n_users, n_cols, rp, np.concatenate(rows))
    assert O.column_counts(wide)[12345] >= 2048          # beyond the 11 spare bits of a word of a 2^20-column catalogue
    prim = rand_csr(rng, n_users, 300, 6, zipf_s=0.8)
    compare_with_oracle(sim_session, [prim, wide], [P(100000, 50), P(100000, 50)], 23)


def test_partition_balances_work(sim_session):
    rng = np.random.default_rng(9)
    work = guarded(torch.from_numpy(rng.zipf(1.5, 5000).astype(np.int64)).to(sim_session.device))
    bounds = sim_session.partition(work, 8)
    assert bounds[0] == 0 and bounds[-1] == 5000 and all(a <= b for a, b in zip(bounds, bounds[1:]))
    pref = np.concatenate([[0], np.cumsum(work.cpu().numpy())])
    total = pref[-1]
    for p in range(1, 8):
        assert pref[bounds[p]] >= total * p // 8 and (bounds[p] == 0 or pref[bounds[p] - 1] < total * p // 8)


def test_partitioned_column_counts_bucket_contiguous_layout(sim_session, monkeypatch):
    """The same with URCCO_COLCOUNT_GLOBAL_LAYOUT=1: the bucket-contiguous form (rounds 1-4; still what catalogues beyond 4M columns take)."""
    monkeypatch.setenv("URCCO_COLCOUNT_GLOBAL_LAYOUT", "1")
    test_partitioned_column_counts_large_matrix(sim_session)


def test_partitioned_column_counts_large_matrix(sim_session):
    """>= 2^20 interactions take the atomic-free partition/dense-LDS histogram (raw counts and, after compaction, the
    post-sampling counts whose length only the device knows): the part-local layout of round 5."""
    rng = np.random.default_rng(10)
    m = rand_csr(rng, 70000, 100_000, 18, zipf_s=1.0)
    assert m.nnz >= (1 << 20)
    dev = sim_session.device
    d = to_dev(m, dev)
    cnt = sim_session.column_counts(d.col_idx, m.nnz, m.n_cols)
    out, post = sim_session.downsample(d, m.nnz, cnt, 11, 40)
    sim_session.synchronize()
    assert np.array_equal(cnt.cpu().numpy(), O.column_counts(m))
    ref = O.downsample(m, O.column_counts(m), 11, 40)
    assert np.array_equal(out.row_ptr.cpu().numpy(), ref.row_ptr)
    assert np.array_equal(out.col_idx.cpu().numpy()[:ref.nnz], ref.col_idx)
    assert np.array_equal(post.cpu().numpy()[:m.n_cols], O.column_counts(ref))
    # unaligned view + a column count that is not a multiple of the bucket size
    buf = torch.zeros(m.nnz + 8, dtype=torch.int32, device=dev)
    view = buf[3:3 + m.nnz]
    view.copy_(d.col_idx[:m.nnz])
    cnt2 = sim_session.column_counts(view, m.nnz, m.n_cols)
    sim_session.synchronize()
    assert np.array_equal(cnt2.cpu().numpy(), O.column_counts(m))


def test_partitioned_column_counts_big_chunks_and_hot_columns(sim_session, monkeypatch):
    """The histogram blocks of matrices beyond URCCO_PH_CHUNK_BIG_NNZ take 61440 ids each and publish 16-bit partial counters: a column
    that fills most of a chunk (count > 32767 inside one block) must survive the packing, with both chunk sizes."""
    rng = np.random.default_rng(14)
    n_users = 75000
    base = rand_csr(rng, n_users, 20_000, 15, zipf_s=1.0)          # its columns move to [16384, 36384): buckets 0 and 1 hold one hot column each
    rows = [np.concatenate([[17, 8200], base.col_idx[base.row_ptr[u]:base.row_ptr[u + 1]] + 16384]) for u in range(n_users)]
    rp = np.zeros(n_users + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    m = O.Csr(n_users, 36_384, rp, np.concatenate(rows).astype(np.int32))
    assert m.nnz >= (1 << 20)
    ref = O.column_counts(m)
    assert ref[17] == n_users and ref[8200] == n_users
    d = to_dev(m, sim_session.device)
    monkeypatch.setenv("URCCO_COLCOUNT_GLOBAL_LAYOUT", "1")
    for big in ("1000000", "2000000000"):
        monkeypatch.setenv("URCCO_PH_CHUNK_BIG_NNZ", big)
        cnt = sim_session.column_counts(d.col_idx, m.nnz, m.n_cols)
        sim_session.synchronize()
        assert np.array_equal(cnt.cpu().numpy(), ref), big
    # the part-local layout: a hot column is one bucket's slice of EVERY part (ranks inside a lane-private copy reach their 10-bit
    # limit when a copy's 1024 ids share a bucket), a length that is not a multiple of the part, and a last bucket of 3616 columns
    monkeypatch.setenv("URCCO_COLCOUNT_GLOBAL_LAYOUT", "0")
    cnt = sim_session.column_counts(d.col_idx, m.nnz, m.n_cols)
    one = O.Csr(1, 36_384, np.array([0, 1 << 20], np.int64), np.full(1 << 20, 20_001, np.int32))  # (not a legal CSR row: the histogram does not care)
    cnt_one = sim_session.column_counts(to_dev(one, sim_session.device).col_idx, one.nnz, one.n_cols)
    sim_session.synchronize()
    assert np.array_equal(cnt.cpu().numpy(), ref)
    assert int(cnt_one[20_001]) == (1 << 20) and int(cnt_one.sum()) == (1 << 20)


def test_large_matrix_full_pipeline(sim_session):
    """>= 2^20 interactions in the primary matrix: partitioned column counts AND the bucketed CSR->CSC feed the SpGEMM;
    the whole build (and an item-range slice, as a multi-GPU rank would run it) still equals the oracle."""
    rng = np.random.default_rng(12)
    a = rand_csr(rng, 90000, 60_000, 13, zipf_s=1.0)
    b = rand_csr(rng, 90000, 300, 3, zipf_s=0.8)
    assert a.nnz >= (1 << 20)
    compare_with_oracle(sim_session, [a, b], [P(30, 8), P(30, 8)], 5)
    compare_with_oracle(sim_session, [a, b], [P(30, 8), P(30, 8)], 5, 0, 20_000, 41_000)


def test_large_transpose_with_item_range(sim_session):
    """urcco_dev_transpose on a large matrix restricted to an item range (what a multi-GPU rank does): columns inside
    the range hold exactly their users (any order), columns outside are empty."""
    rng = np.random.default_rng(13)
    m = rand_csr(rng, 80000, 30_000, 15, zipf_s=0.9)
    assert m.nnz >= (1 << 20)
    dev = sim_session.device
    d = to_dev(m, dev)
    counts = guarded(torch.from_numpy(O.column_counts(m)).to(dev))
    cp_ref, ri_ref = O.transpose(m)
    for lo, hi in [(0, m.n_cols), (9000, 17123)]:
        cp, ri = sim_session.transpose(d, counts, lo, hi)
        sim_session.synchronize()
        cp, ri = cp.cpu().numpy(), ri.cpu().numpy()
        lens = np.diff(cp)
        expect = np.diff(cp_ref).copy()
        expect[:lo] = 0
        expect[hi:] = 0
        assert np.array_equal(lens, expect)
        for j in list(range(lo, min(lo + 50, hi))) + [hi - 1] + rng.integers(lo, hi, 200).tolist():
            assert np.array_equal(np.sort(ri[cp[j]:cp[j + 1]]), ri_ref[cp_ref[j]:cp_ref[j + 1]])


def test_large_transpose_long_rows_and_empty_parts(sim_session):
    """The two-level transposition's parts (flat runs of 16384 entries since round 6): rows longer than a part (several parts inside one row),
    runs of empty rows, a ragged last part; every column compared."""
    rng = np.random.default_rng(14)
    lengths = rng.poisson(19, 70000)
    lengths[rng.random(70000) < 0.2] = 0
    lengths[100] = 25_000          # a row over more than one part
    lengths[101] = 17_000
    lengths[40_000:40_300] = 0
    lengths[69_999] = 20_000       # the last part ends in a long row
    m = _csr_from_lengths(rng, lengths, 50_000)
    assert m.nnz >= (1 << 20)
    dev = sim_session.device
    d = to_dev(m, dev)
    counts = guarded(torch.from_numpy(O.column_counts(m)).to(dev))
    cp_ref, ri_ref = O.transpose(m)
    for lo, hi in [(0, m.n_cols), (123, 45_678)]:
        cp, ri = sim_session.transpose(d, counts, lo, hi)
        sim_session.synchronize()
        cp, ri = cp.cpu().numpy(), ri.cpu().numpy()
        expect = np.diff(cp_ref).copy()
        expect[:lo] = 0
        expect[hi:] = 0
        assert np.array_equal(np.diff(cp), expect)
        for j in range(lo, hi):
            assert np.array_equal(np.sort(ri[cp[j]:cp[j + 1]]), ri_ref[cp_ref[j]:cp_ref[j + 1]]), j


def test_large_transpose_long_runs_of_empty_rows(sim_session):
    """Round 6's part-local transposition finds an entry's row from 16-bit marks of the part's row starts; a part whose row slice holds more
    than 65536 rows (a long run of users without a single kept interaction) takes the binary-search form instead.  Every column compared."""
    rng = np.random.default_rng(16)
    lengths = rng.poisson(11, 200_000)
    lengths[50_000:120_100] = 0          # 70 100 empty rows inside one part
    lengths[120_100] = 3
    lengths[0] = 0
    lengths[199_990:] = 0                # empty rows behind the last entry
    m = _csr_from_lengths(rng, lengths, 40_000)
    assert m.nnz >= (1 << 20)
    dev = sim_session.device
    d = to_dev(m, dev)
    counts = guarded(torch.from_numpy(O.column_counts(m)).to(dev))
    cp_ref, ri_ref = O.transpose(m)
    for lo, hi in [(0, m.n_cols), (1000, 39_000)]:
        cp, ri = sim_session.transpose(d, counts, lo, hi)
        sim_session.synchronize()
        cp, ri = cp.cpu().numpy(), ri.cpu().numpy()
        expect = np.diff(cp_ref).copy()
        expect[:lo] = 0
        expect[hi:] = 0
        assert np.array_equal(np.diff(cp), expect)
        for j in range(lo, hi):
            assert np.array_equal(np.sort(ri[cp[j]:cp[j + 1]]), ri_ref[cp_ref[j]:cp_ref[j + 1]]), j


def test_large_transpose_skewed_ids_heavy_bucket(sim_session):
    """Ids that follow popularity (what first-appearance ids do): nearly every interaction falls into the first column bucket,
    which is then placed by several blocks sharing cursors in global memory instead of one block with LDS cursors."""
    rng = np.random.default_rng(15)
    n_rows, n_cols = 300_000, 30_000
    hot = np.sort(rng.integers(0, 60, size=(n_rows, 6)), axis=1)
    rows = []
    for r in range(n_rows):
        c = np.unique(hot[r])
        if r % 50 == 0:
            c = np.unique(np.concatenate([c, rng.integers(60, n_cols, 3)]))
        rows.append(c)
    rp = np.zeros(n_rows + 1, np.int64)
    np.cumsum([len(c) for c in rows], out=rp[1:])
    m = O.Csr(n_rows, n_cols, rp, np.concatenate(rows).astype(np.int32))
    assert m.nnz >= (1 << 20)
    dev = sim_session.device
    counts = guarded(torch.from_numpy(O.column_counts(m)).to(dev))
    cp_ref, ri_ref = O.transpose(m)
    cp, ri = sim_session.transpose(to_dev(m, dev), counts, 0, n_cols)
    sim_session.synchronize()
    cp, ri = cp.cpu().numpy(), ri.cpu().numpy()
    assert np.array_equal(cp, cp_ref)
    for j in list(range(0, 70)) + rng.integers(60, n_cols, 300).tolist():
        assert np.array_equal(np.sort(ri[cp[j]:cp[j + 1]]), ri_ref[cp_ref[j]:cp_ref[j + 1]]), j


@pytest.mark.parametrize("wire", ["u16", "i32"])
def test_merge_of_csc_fragments(sim_session, wire):
    """urcco_dev_merge_fragments (multi-GPU: every rank transposes its own user shard, a rank's item range arrives as W fragments):
    fragments made with the library's own transposition of uneven shards (one of them empty), merged for every range of a
    3-way split, against the CSC of the whole matrix (global user ids)."""
    sess = sim_session
    dev = sess.device
    rng = np.random.default_rng(21)
    n_users, n_items = 5000, 700
    m = rand_csr(rng, n_users, n_items, 11, zipf_s=1.1)
    cuts = [0, 1700, 1700, 4100, n_users]                    # W = 4, shard 1 is empty
    W = len(cuts) - 1
    counts = O.column_counts(m)
    csc_cp = np.zeros(n_items + 1, np.int64)
    np.cumsum(counts, out=csc_cp[1:])
    order = np.argsort(m.col_idx, kind="stable")
    csc_ri = np.repeat(np.arange(n_users), np.diff(m.row_ptr))[order]
    frags = []
    for lo, hi in zip(cuts, cuts[1:]):
        sh = O.Csr(hi - lo, n_items, m.row_ptr[lo:hi + 1] - m.row_ptr[lo], m.col_idx[m.row_ptr[lo]:m.row_ptr[hi]])
        l_cnt = O.column_counts(sh)
        cp, ri = sess.transpose(to_dev(sh, dev), guarded(torch.from_numpy(l_cnt).to(dev)))
        frags.append((l_cnt, cp.cpu().numpy(), ri.cpu().numpy()))
    sizes = np.zeros(_lib.EXCH_SIZES * W, np.int64)          # (rows, nnz, long rows, counts that do not fit a packed word) per shard
    sizes[0::_lib.EXCH_SIZES] = np.diff(cuts)
    bounds = [0, 90, 90 + 333, n_items]
    for lo, hi in zip(bounds, bounds[1:]):
        lens = np.concatenate([f[0][lo:hi] for f in frags])
        ents = np.concatenate([f[2][f[1][lo]:f[1][hi]] for f in frags]).astype(np.int32)
        lens_t = torch.from_numpy(lens.astype(np.uint16) if wire == "u16" else lens.astype(np.int32))
        cp, ri = sess.merge_fragments(W, lo, hi, n_items, guarded(lens_t.to(dev)), guarded(torch.from_numpy(np.concatenate([ents, np.zeros(1, np.int32)])).to(dev)),
                                      int(ents.size), guarded(torch.from_numpy(sizes).to(dev)), guarded(torch.from_numpy(counts).to(dev)))
        cp, ri = cp.cpu().numpy(), ri.cpu().numpy()
        ref_cp = np.zeros(n_items + 1, np.int64)
        np.cumsum(np.where((np.arange(n_items) >= lo) & (np.arange(n_items) < hi), counts, 0), out=ref_cp[1:])
        assert np.array_equal(cp, ref_cp)
        got = ri[: ref_cp[-1]].copy()
        for j in range(lo, hi):                                # the library's transposition does not order a column; a fragment's run stays together
            got[ref_cp[j]:ref_cp[j + 1]].sort()
        assert np.array_equal(got, csc_ri[csc_cp[lo]:csc_cp[hi]])


def _csr_from_lengths(rng, lengths, n_cols):
    lengths = np.asarray(lengths, dtype=np.int64)
    rp = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=rp[1:])
    ci = np.empty(int(rp[-1]), dtype=np.int32)
    for r, n in enumerate(lengths):
        if n:
            ci[rp[r]:rp[r + 1]] = np.sort(rng.choice(n_cols, size=int(n), replace=False))
    return O.Csr(len(lengths), n_cols, rp, ci)


@pytest.mark.parametrize("mode", [0, 1])
def test_row_scan_tile_edges(sim_session, mode):
    """sampleDownAndBinarize shapes that stress the tiled scan: runs of empty rows longer than the staged row_ptr
    slice, rows longer than a tile (and than maxElementsPerRow: Int/Int rate 0 vs fractional), leading / trailing
    empty rows, a tile boundary that coincides with a row boundary, a last partial tile."""
    rng = np.random.default_rng(21 + mode)
    n_cols = 20000
    lengths = ([0] * 7 + [4096] + [0] * 6000 + [3, 0, 0, 5] + [9000] + [0] * 3 + [1] * 5000 + [0] * 4500 + [700, 2, 0, 11, 4093]
               + list(rng.integers(0, 40, 3000)) + [0] * 9)
    m = _csr_from_lengths(rng, lengths, n_cols)
    dev = sim_session.device
    raw_ref = O.column_counts(m)
    raw = guarded(torch.from_numpy(raw_ref).to(dev))
    for max_n in (3, 500):
        out, post = sim_session.downsample(to_dev(m, dev), m.nnz, raw, 99, max_n, mode)
        sim_session.synchronize()
        ref = O.downsample(m, raw_ref, 99, max_n, mode)
        assert np.array_equal(out.row_ptr.cpu().numpy(), ref.row_ptr)
        assert np.array_equal(out.col_idx.cpu().numpy()[:ref.nnz], ref.col_idx)
        assert np.array_equal(post.cpu().numpy()[:n_cols], O.column_counts(ref))


def test_all_equal_llr_ties_cut_by_column(sim_session):
    """Every candidate of a row has the same LLR and there are more of them than k: the radix select finds no
    differing key byte and the cut is decided by the column order alone (llr desc, col asc).  A second block of
    items shares only the exponent bytes.  A third matrix puts such rows into the micro class (one wave, ranking by counting).  Exact ids."""
    rng = np.random.default_rng(17)
    n_users, n_items = 900, 300
    rows = []
    for u in range(n_users):
        if u < 120:
            rows.append(np.arange(0, 200))                  # block 1: 200 items always together -> identical LLR
        elif u < 400:
            rows.append(np.sort(rng.choice(np.arange(200, 300), size=12, replace=False)))
        else:
            rows.append(np.zeros(0, np.int64))
    lengths = [len(r) for r in rows]
    rp = np.zeros(n_users + 1, np.int64)
    np.cumsum(lengths, out=rp[1:])
    ci = np.concatenate(rows).astype(np.int32)
    a = O.Csr(n_users, n_items, rp, ci)
    for k in (5, 50, 64, 150):
        _, _, stats = compare_with_oracle(sim_session, [a, a], [P(100000, k), P(100000, k)], 3, exact_ids=True)
    # the same in the micro class: 3 users hold the same 20 items and nothing else (cA = 3, w = 60 pairs): every row has 19 candidates of one LLR
    m = _tied_block(40, 64, 3, np.arange(7, 27))
    for k in (5, 19, 50):
        out, _, stats = compare_with_oracle(sim_session, [m, m], [P(100000, k), P(100000, k)], 3, exact_ids=True)
        assert int(stats[0][0][1]) == 20 and int(stats[1][0][1]) == 20, stats[0][0][1:8]
        assert [int(np.diff(o.to_host()[0]).max()) for o in out] == [min(k, 19), min(k, 20)]


def _tied_block(n_users, n_items, holders, block, extra_rows=()):
    """`holders` users each hold every item of `block`; extra_rows = [(user, items)] of further interactions."""
    rows = [np.zeros(0, np.int64) for _ in range(n_users)]
    for u in range(holders):
        rows[u] = np.asarray(block, np.int64)
    for u, items in extra_rows:
        rows[u] = np.union1d(rows[u], np.asarray(items, np.int64))
    rp = np.zeros(n_users + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    return O.Csr(n_users, n_items, rp, np.concatenate(rows).astype(np.int32))


def test_many_ties_at_the_cut_after_skipped_column_passes(sim_session):
    """Radix select, column passes: more than SEL_M candidates tied exactly at the k boundary, so the cut is decided in
    the COLUMN digits -- reached after the constant high column bytes were skipped.  The rotating histograms must be
    indexed by executed pass, not by digit position (round-1 defect: a stale histogram truncated these rows).  Covers
    col_bytes 1 / 3 for the one-wave class (two histograms) and col_bytes 2 for the 256-/512-thread classes (three),
    with several N so that the LLR's low byte lands on both sides of the cut digit.  Exact ids."""
    # one-wave class, col_bytes = 1: 150 items always together, 2 users (w = 300), k = 20
    for n_users in (11, 12, 13, 17, 23, 31, 57, 101):
        a = _tied_block(n_users, 150, 2, np.arange(150))
        _, _, st = compare_with_oracle(sim_session, [a, a], [P(100000, 20), P(100000, 20)], 3, exact_ids=True)
        assert st[1][0][2] > 0          # wave class used
    # one-wave class, col_bytes = 3 (hash-addressed table): the tied columns sit above 2^16
    for n_users in (11, 13, 29, 64):
        cols = 70000 + 3 * np.arange(150)
        b = _tied_block(n_users, 70600, 2, cols)
        a = _tied_block(n_users, 150, 2, np.arange(150))
        compare_with_oracle(sim_session, [a, b], [P(100000, 20), P(100000, 20)], 3, exact_ids=True)
    # 512-thread class, col_bytes = 2: 1000 tied columns at 30000..30999, 3 users (w = 3000), k = 50
    for n_users in (7, 9, 14, 33):
        a = _tied_block(n_users, 40000, 3, np.arange(30000, 31000))
        _, _, st = compare_with_oracle(sim_session, [a, a], [P(100000, 50), P(100000, 50)], 3, exact_ids=True)
        assert st[1][0][5] > 0          # half-CU class used
    # 256-thread class (tracks shared key bytes): a second LLR value below the tied block keeps the key passes alive
    for n_users in (9, 15, 40):
        extra = [(5, np.arange(20000, 20040)), (6, np.arange(20000, 20040))]
        a = _tied_block(n_users, 40000, 2, np.arange(30000, 30400), extra_rows=[(0, np.arange(20000, 20040))] + extra)
        _, _, st = compare_with_oracle(sim_session, [a, a], [P(100000, 50), P(100000, 50)], 3, exact_ids=True)
        assert st[1][0][3] + st[1][0][4] > 0


def test_row_scan_threshold_table_forms(sim_session):
    """sampleDownAndBinarize over three column-space regimes: a few thousand sampled ("hot") columns carrying most of the
    interactions, nearly every column sampled, and a wide sparse column space.  Both row-rate modes.  (Written for the
    LDS-resident threshold tables tried in round 2 -- measured no faster than the L2 gather and removed -- and kept as a
    regression net for any later form of the keep decision.)"""
    rng = np.random.default_rng(33)
    dev = sim_session.device
    cases = [(rand_csr(rng, 60000, 30000, 25, zipf_s=1.0), 20),        # (a) ~2K hot columns carrying most interactions
             (rand_csr(rng, 20000, 60000, 60, zipf_s=0.3), 3),          # (b) nearly every one of 60K columns is hot
             (rand_csr(rng, 30000, 400000, 40, zipf_s=0.9), 5)]         # (c) 400K columns: bitmap does not fit
    for m, max_n in cases:
        raw_ref = O.column_counts(m)
        raw = guarded(torch.from_numpy(raw_ref).to(dev))
        for mode in (0, 1):
            out, post = sim_session.downsample(to_dev(m, dev), m.nnz, raw, 1234, max_n, mode)
            sim_session.synchronize()
            ref = O.downsample(m, raw_ref, 1234, max_n, mode)
            assert np.array_equal(out.row_ptr.cpu().numpy(), ref.row_ptr)
            assert np.array_equal(out.col_idx.cpu().numpy()[:ref.nnz], ref.col_idx)
            assert np.array_equal(post.cpu().numpy()[:m.n_cols], O.column_counts(ref))


def test_global_class_ties_at_the_cut(sim_session):
    """Bin 6 reached through the packed-count overflow (3M columns leave 10 count bits, the item has 1100 users).  At k <= 256 -- every k
    here -- bin 6 is the MULTI-PASS class (the dense global-accumulator kernel serves it only from k = 257 on: tests/large_k_cases.py): 200
    candidates with exactly equal LLR, so the cut falls in the column digits (3 column bytes).  Exact ids."""
    n_users, n_b = 1300, 3_000_000
    a_rows = [np.array([0], np.int64) if u < 1100 else np.array([1], np.int64) for u in range(n_users)]
    cols = 70000 + 3 * np.arange(200)
    b_rows = [cols if u < 1100 else np.array([5, 2_999_999], np.int64) for u in range(n_users)]
    def csr(rows, n_cols):
        rp = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=rp[1:])
        return O.Csr(len(rows), n_cols, rp, np.concatenate(rows).astype(np.int32))
    a, b = csr(a_rows, 2), csr(b_rows, n_b)
    for k in (7, 50, 150):
        _, _, st = compare_with_oracle(sim_session, [a, b], [P(1000000, k), P(1000000, k)], 3, exact_ids=True)
        assert st[1][0][7] > 0          # bin 6 used


def test_multipass_class_adversarial_low_bits_and_k_limits(sim_session):
    """The multi-pass class (bin 6) partitions a row's columns by their LOW bits.  Here every column the heavy rows touch is a
    multiple of 8, so the first partitions are empty or overflowing and the row has to start over with twice the passes several
    times (P = 2, 4, 8 leave everything in pass 0; P = 16 splits it).  k = 256 is the largest the class keeps running lists for;
    k = 257 takes the dense global-accumulator kernel instead: both must equal the oracle, ids exact."""
    rng = np.random.default_rng(21)
    n_users, n_b = 700, 200_000
    a = rand_csr(rng, n_users, 3, 2, zipf_s=2.0)                    # three items, item 0 owned by most users
    cols = np.sort(rng.choice(n_b // 8, size=15_000, replace=False)).astype(np.int64) * 8
    b_rows = []
    for u in range(n_users):
        pick = np.sort(rng.choice(cols.size, size=120, replace=False))
        b_rows.append(cols[pick])
    rp = np.zeros(n_users + 1, np.int64)
    np.cumsum([len(r) for r in b_rows], out=rp[1:])
    b = O.Csr(n_users, n_b, rp, np.concatenate(b_rows).astype(np.int32))
    for k in (50, 256, 257):
        _, _, st = compare_with_oracle(sim_session, [a, b], [P(1000000, k), P(1000000, k)], 9)
        assert st[1][0][7] > 0, st[1][0]                            # bin 6 used for A'B


@pytest.mark.parametrize("mode", [0, 1])
def test_row_scan_large_matrix_edges(sim_session, mode):
    """The row scan on matrices of >= 2^20 interactions (post-sampling counts through the partitioned histogram): runs of empty
    rows across tile boundaries, rows beyond the interaction cap (both row-rate modes), a row spanning several tiles, trailing
    empty rows, and an interaction count that is an exact multiple of the tile -- row_ptr and col_idx bit for bit against the
    oracle."""
    rng = np.random.default_rng(31 + mode)
    for exact in (False, True):
        lengths = rng.poisson(17, 80_000)
        lengths[rng.random(80_000) < 0.15] = 0
        lengths[5_000:5_700] = 0                     # 700 empty rows in a row
        lengths[123] = 9_000                         # spans three tiles, > max_n
        lengths[40_000] = 300                        # > max_n inside a tile
        lengths[79_990:] = 0                         # trailing empty rows
        total = int(lengths.sum())
        assert total >= (1 << 20)
        if exact:
            lengths[77_777] += (-total) % 4096       # nnz becomes a multiple of the tile size
        m = _csr_from_lengths(rng, lengths, 30_000)
        assert (m.nnz % 4096 == 0) == exact
        dev = sim_session.device
        raw_ref = O.column_counts(m)
        raw = guarded(torch.from_numpy(raw_ref).to(dev))
        ref = O.downsample(m, raw_ref, 4242, 200, mode)
        out, post = sim_session.downsample(to_dev(m, dev), m.nnz, raw, 4242, 200, mode)
        sim_session.synchronize()
        assert np.array_equal(out.row_ptr.cpu().numpy(), ref.row_ptr)
        assert np.array_equal(out.col_idx.cpu().numpy()[:ref.nnz], ref.col_idx)
        assert np.array_equal(post.cpu().numpy()[:m.n_cols], O.column_counts(ref))


def test_select_ambiguous_set_overlays_the_histograms(sim_session):
    """The workload of the round-3 race (helpers.select_race_workload): 120 candidates tied at the top LLR (+ 100 weaker ones) per row in the 256-thread
    small-block class, whose LDS layout overlays the ambiguous set on the select histograms.  The simulator runs the waves of a
    team one after the other between rendezvous, so it cannot interleave them as the race needs (the -m gpu test runs the same
    build with a wave delayed on hardware); here the logic of the path -- and of the barrier round 4 added -- is checked with exact ids, delay hook on."""
    from helpers import SELECT_RACE_ROWS_SMALL_BLOCK, select_race_workload
    sim_session.set_debug(_lib.DBG_SELECT_DELAY)
    try:
        _, _, stats = compare_with_oracle(sim_session, select_race_workload(), [P(), P()], 77, exact_ids=True)
    finally:
        sim_session.set_debug(0)
    assert all(int(s[0][1 + 2]) == SELECT_RACE_ROWS_SMALL_BLOCK for s in stats)


# ---- catalogue widths at which the code path changes (tests/test_gpu_wide_catalogues.py runs these on hardware) ----------------------
# > 4,194,304 columns (PL_MAX_BUCKETS x 16384): column counts leave the part-local layout for the bucket-contiguous one; > 8,388,608 (PH_MAX_BUCKETS x
# 8192, TP_MAX_BUCKETS x 16384): the atomic column-count kernel, post-sampling counts by L2 atomics inside the row scan, the cursor-atomic transposition.
LAYOUT_WIDTHS = [4_194_304, 4_194_305, 8_388_608, 8_388_609]


def csr_from_pairs(n_rows, n_cols, users, cols):
    """Binary CSR of the (user, column) pairs, duplicates merged."""
    key = np.unique(np.asarray(users, np.int64) * n_cols + np.asarray(cols, np.int64))
    u = key // n_cols
    rp = np.zeros(n_rows + 1, np.int64)
    np.cumsum(np.bincount(u, minlength=n_rows), out=rp[1:])
    return O.Csr(n_rows, n_cols, rp, (key - u * n_cols).astype(np.int32))


def wide_pairs(rng, n_rows, n_cols, avg, head=2000, first_appearance=False):
    """(users, cols) of Poisson(avg) entries per row over a catalogue too wide for a dense CDF (rand_csr): half the entries from a Zipf head
    of `head` ids -- the first ids (first-appearance, i.e. popularity-ordered ids) or scattered over the width -- the rest uniform."""
    deg = rng.poisson(avg, n_rows)
    total = int(deg.sum())
    if first_appearance:
        ids = np.arange(head, dtype=np.int64)
    else:
        ids = rng.permutation(np.unique(rng.integers(0, n_cols, 2 * head)))[:head]
    r = np.minimum(rng.zipf(1.2, total) - 1, ids.size - 1)
    cols = np.where(rng.random(total) < 0.5, ids[r], rng.integers(0, n_cols, total))
    return np.repeat(np.arange(n_rows, dtype=np.int64), deg), cols


def _csc_as_sets(cp, ri):
    """Row indices of a CSC sorted inside every column: the cursor-atomic transposition writes a column's rows in any order."""
    col = np.repeat(np.arange(cp.size - 1, dtype=np.int64), np.diff(cp))
    return ri[np.lexsort((ri, col))]


def column_layout_boundary_case(sess, n_cols):
    """Column counts, both row-rate modes under both RNGs, and the transposition of the raw and the down-sampled matrix at a catalogue width
    where the code path changes (LAYOUT_WIDTHS), against the oracle: >= 2^20 entries, two columns held by 40,000 users (more than a 16-bit
    partial counter holds), first-appearance ids that crowd the first buckets and ids scattered up to the last column.  The CSC is compared
    per column as a set."""
    R = O.RNG_MIX32
    rng = np.random.default_rng(n_cols % 1000)
    n_users = 70_000
    u1, c1 = wide_pairs(rng, n_users, n_cols, 9, first_appearance=True)
    u2, c2 = wide_pairs(rng, n_users, n_cols, 8)
    hot_u = rng.choice(n_users, 40_000, replace=False)
    users = np.concatenate([u1, u2, hot_u, hot_u, np.full(3, 17)])
    cols = np.concatenate([c1, c2, np.zeros(40_000, np.int64), np.full(40_000, n_cols - 1), [n_cols - 2, n_cols // 2, (n_cols - 1) & ~16383]])
    m = csr_from_pairs(n_users, n_cols, users, cols)
    assert m.nnz >= (1 << 20)
    raw_ref = O.column_counts(m)
    assert raw_ref[0] >= 40_000 and raw_ref[n_cols - 1] >= 40_000
    d = to_dev(m, sess.device)
    cnt = sess.column_counts(d.col_idx, m.nnz, n_cols)
    cp, ri = sess.transpose(d, cnt)
    sess.synchronize()
    assert np.array_equal(cnt.cpu().numpy(), raw_ref), "raw column counts differ"
    ref_cp, ref_ri = O.transpose(m)
    assert np.array_equal(cp.cpu().numpy(), ref_cp), "col_ptr of the raw matrix differs"
    assert np.array_equal(_csc_as_sets(ref_cp, ri[:m.nnz].cpu().numpy()), _csc_as_sets(ref_cp, ref_ri)), "CSC of the raw matrix differs"
    for mode in (0, 1, R, R | 1):
        out, post = sess.downsample(d, m.nnz, cnt, 29, 40, mode)
        sess.synchronize()
        ref = O.downsample(m, raw_ref, 29, 40, mode)
        assert np.array_equal(out.row_ptr.cpu().numpy(), ref.row_ptr), mode
        assert np.array_equal(out.col_idx.cpu().numpy()[:ref.nnz], ref.col_idx), mode
        post_ref = O.column_counts(ref)
        assert np.array_equal(post.cpu().numpy()[:n_cols], post_ref), mode
        if mode == (R | 1):
            cp, ri = sess.transpose(out, post)
            sess.synchronize()
            ref_cp, ref_ri = O.transpose(ref)
            assert np.array_equal(cp.cpu().numpy(), ref_cp), "col_ptr of the down-sampled matrix differs"
            assert np.array_equal(_csc_as_sets(ref_cp, ri[:ref.nnz].cpu().numpy()), _csc_as_sets(ref_cp, ref_ri)), "CSC of the down-sampled matrix differs"


@pytest.mark.parametrize("n_cols", LAYOUT_WIDTHS)
def test_column_layout_boundaries(sim_session, n_cols):
    column_layout_boundary_case(sim_session, n_cols)


# Ties cut in the column digits at every col_bytes: widths just below and above each byte boundary of a column index.
TIE_WIDTHS = [256, 257, 65_536, 65_537, 1 << 24, (1 << 24) + 1]


def tied_columns(n_cols, n):
    """n columns of B for a row whose candidates all tie: three small columns, columns spread over every value of the highest column digit
    below 2^24 (so that the first column pass -- of the highest digit this width uses -- leaves fewer than k candidates in the top bin and
    the cut falls in a lower bin), and the multiples of the highest used byte's unit below the width (columns that differ from 0 only in that
    digit: 2^24 at 2^24 + 1 columns)."""
    col_bytes = 1 if n_cols <= (1 << 8) else (2 if n_cols <= (1 << 16) else (3 if n_cols <= (1 << 24) else 4))
    if col_bytes == 1:
        return np.arange(n_cols - n, n_cols)
    unit = 1 << (8 * (col_bytes - 1))
    tops = [unit * j for j in range(1, 4) if unit * j < n_cols]
    lo, hi = 1 << (8 * (min(col_bytes, 3) - 1)), min(n_cols, 1 << 24)
    spread = np.linspace(lo, hi - 1, max(n - 3 - len(tops), 1)).astype(np.int64) if hi > lo else np.zeros(0, np.int64)
    cols = np.unique(np.concatenate([[1, 2, 3], spread, tops]))
    return np.union1d(cols, np.setdiff1d(np.arange(4, 4 + n), cols)[:max(n - cols.size, 0)])


def tie_cases(n_cols):
    """(holders, tied columns, k, accumulator class of the row): micro, one wave, small block / block, and bin 6 -- by the table's capacity
    (multi-pass; k = 257: the global kernel) or, from 2^24 columns on (7 count bits), by the packed-count rule at cA = 128."""
    cases = [(2, 30, 5, 0), (2, 150, 20, 1)]
    if n_cols <= 257:
        return cases + [(4, 200, 50, 2)]
    cases += [(2, 1000, 50, 3), (2, 11_000, 50, 6), (2, 11_000, 257, 6)]
    if n_cols >= (1 << 24):
        cases += [(127, 60, 50, 5), (128, 60, 50, 6), (128, 300, 257, 6)]
    return cases


def column_digit_ties_case(sess, n_cols):
    """Rows with more than k candidates of exactly equal LLR (the holders of the row's item hold exactly the same tied columns and nothing
    else), so that the cut is decided in the column digits alone, down to the highest byte a column index of this width uses.  Exact ids;
    the row must land in the intended accumulator class."""
    for holders, n_tied, k, cls in tie_cases(n_cols):
        cols = tied_columns(n_cols, n_tied)
        assert cols.size > k and cols.max() < n_cols
        n_users = holders + 40
        a = csr_from_pairs(n_users, 2, np.concatenate([np.arange(holders), np.arange(holders, holders + 10)]),
                           np.concatenate([np.zeros(holders, np.int64), np.ones(10, np.int64)]))
        b = csr_from_pairs(n_users, n_cols, np.repeat(np.arange(holders), cols.size), np.tile(cols, holders))
        _, _, st = compare_with_oracle(sess, [a, b], [P(100000, k), P(100000, k)], 5, exact_ids=True)
        rows = st[1][0][1:8]
        assert rows[cls] == 1 and rows.sum() == 1, (n_cols, holders, cols.size, k, rows)


@pytest.mark.parametrize("n_cols", TIE_WIDTHS)
def test_ties_cut_in_the_highest_column_digit(sim_session, n_cols):
    column_digit_ties_case(sim_session, n_cols)
