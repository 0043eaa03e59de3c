"""Whole model builds at the catalogue widths where the code path changes, on a real MI355X (-m gpu).

The width of B picks the packed accumulator's count bits (cco_rows.hip choose_bin: a row whose cA does not fit them goes to bin 6) and the
column digits the top-k tie cut reads (col_bytes); the width of A picks the column-count layout and the transposition.  The stage-level
cases at these widths (and the ties cut in every column digit) are tests/test_sim_kernel_logic.py cases, run on hardware by
tests/test_gpu_parity.py."""
import numpy as np
import pytest
import torch

from helpers import compare_with_oracle, compare_with_oracle_large, rand_csr, run_device, to_dev, to_params
from oracle import c_oracle as O
from test_sim_kernel_logic import csr_from_pairs, wide_pairs
from universal_recommender_amd import _lib
from universal_recommender_amd import device as D

pytestmark = pytest.mark.gpu

NBINS = 7
A_WIDTH = 8_388_609                                                        # beyond 8M: atomic counts, cursor-atomic transposition of A
B_WIDTHS = [16_777_215, 16_777_216, 16_777_217, (1 << 25) + 1]            # key_bits 24 / 25 (col_bytes 3) / 25 (col_bytes 4) / 26
CUT_HOLDERS = [63, 64, 65, 127, 128, 129, 255, 256, 257]                  # cA just below, at and above the cuts of 6, 7 and 8 count bits
ORACLE_THREADS = 16


def count_bits(n_cols_b):
    return 32 - int(n_cols_b).bit_length()            # the bits a packed (column + 1, count) word leaves for the count


def expected_bins(a, b, n_cols_b, k):
    """Rows and users (sum of cA) per accumulator class of A'B, from the oracle's down-sampled A and B: the binning rule of cco_rows.hip
    (choose_bin) -- cA beyond the count bits -> bin 6; micro; else the larger of the class the table size needs and the class the work wants."""
    w = np.bincount(a.col_idx, weights=np.repeat(np.diff(b.row_ptr), np.diff(a.row_ptr)).astype(np.float64), minlength=a.n_cols).astype(np.int64)
    ca = np.bincount(a.col_idx, minlength=a.n_cols).astype(np.int64)
    live = (w > 0) & (ca > 0)
    w, ca = w[live], ca[live]
    dmax = np.minimum(w, n_cols_b) * 3 + 3 * k + 2
    cap = np.select([dmax <= 1024, dmax <= 4096, dmax <= 8192, dmax <= 16384, dmax <= 32768], [1, 2, 3, 4, 5], 6)
    work = np.select([w <= 512, w <= 8192], [1, 2], 4)
    cls = np.maximum(cap, work)
    cls[(w <= 64) & (ca <= 64)] = 0
    cb = count_bits(n_cols_b)
    if cb < 31:
        cls[ca > (1 << cb) - 1] = 6
    return np.bincount(cls, minlength=NBINS), np.bincount(cls, weights=ca.astype(np.float64), minlength=NBINS).astype(np.int64)


def snapshot(outs):
    """Bits of every indicator matrix of a build: row_ptr, ids, LLR bytes, the stats vector."""
    res = []
    for o in outs:
        rp, ci, llr = o.to_host()
        res.append((rp.copy(), ci.copy(), np.ascontiguousarray(llr).view(np.uint64).copy(), o.stats.cpu().numpy().copy()))
    return res


def assert_same_bits(x, y, label):
    for d, (p, q) in enumerate(zip(x, y)):
        for name, u, v in zip(("row_ptr", "ids", "LLR bits", "stats"), p, q):
            assert np.array_equal(u, v), f"{label}, event {d}: {name} differ"


def _wide_job(seed):
    """A of 8,388,609 items and the four Bs; 250,000 users.  Down-sampling bites (a column of 6,000 users, users of 700 interactions, caps
    of 300); items held by exactly CUT_HOLDERS users who hold nothing else in A and one column of each B, so their post-sampling cA is exact
    and their work w = cA."""
    rng = np.random.default_rng(seed)
    n_users, n_ctl = 250_000, sum(CUT_HOLDERS)
    n_base = n_users - n_ctl
    ctl_items = A_WIDTH - 1 - 7 * np.arange(len(CUT_HOLDERS))
    ctl_users = n_base + np.arange(n_ctl)

    def matrix(n_cols, avg, ctl_cols, first_appearance):
        u, c = wide_pairs(rng, n_base, n_cols, avg, first_appearance=first_appearance)
        heavy = rng.choice(n_base, 20, replace=False)
        hot_u = rng.choice(n_base, 6000, replace=False)
        users = np.concatenate([u, np.repeat(heavy, 700), hot_u, ctl_users])
        cols = np.concatenate([c, rng.integers(0, n_cols, 20 * 700), np.full(6000, 5), ctl_cols])
        if n_cols == A_WIDTH:
            cols[:u.size + 20 * 700][np.isin(cols[:u.size + 20 * 700], ctl_items)] = 1     # the controlled items keep exactly their holders
        return csr_from_pairs(n_users, n_cols, users, cols)

    a = matrix(A_WIDTH, 4, np.repeat(ctl_items, CUT_HOLDERS), True)
    bs = [matrix(w, 5, rng.integers(0, w, n_ctl), False) for w in B_WIDTHS]
    return [a] + bs


def test_whole_builds_at_wide_catalogues(gpu_session):
    """A at 8,388,609 items, Bs at 16,777,215 / 16,777,216 / 16,777,217 / 2^25 + 1 columns: the session path and the context path against the
    C oracle (down-sampled matrices bit for bit, every indicator row).  Rows and users per accumulator class equal the binning rule applied
    to the oracle's matrices, so the items at cA = 2^count_bits land in bin 6 and those one below do not.  Repeated builds, and builds
    with plain B' words plus the count gather (debug 1048576 / pack_counts off), are bit-identical to the first."""
    mats = _wide_job(8_388_609)
    params = [O.DatasetParams(300, 50, None)] * len(mats)
    mode, seed = _lib.ROW_RATE_FRACTIONAL, 77
    dev_mats = [to_dev(m, gpu_session.device) for m in mats]
    ctx = D.Context(gpu_session.device, gpu_session.lib, 1, 0, mode)
    try:
        first = snapshot(D.cross_occurrence_context(ctx, dev_mats, to_params(params), seed))
        assert_same_bits(snapshot(D.cross_occurrence_context(ctx, dev_mats, to_params(params), seed)), first, "context, second build")
        ctx.set_debug(_lib.DBG_UNPACKED_COUNTS)
        assert_same_bits(snapshot(D.cross_occurrence_context(ctx, dev_mats, to_params(params), seed)), first, "context, count gather")
        ctx.set_debug(0)
        ctx_out = D.cross_occurrence_context(ctx, dev_mats, to_params(params), seed)
        out, res = compare_with_oracle_large(gpu_session, mats, params, seed, mode, threads=ORACLE_THREADS, dev_mats=dev_mats, also=[("context", ctx_out)])
    finally:
        ctx.close()
    assert_same_bits(snapshot(out), first, "session vs context")
    assert_same_bits(snapshot(D.cross_occurrence_device(gpu_session, dev_mats, to_params(params), seed, mode)), first, "session, second build")
    gpu_session.pack_counts = False
    try:
        assert_same_bits(snapshot(D.cross_occurrence_device(gpu_session, dev_mats, to_params(params), seed, mode)), first, "session, count gather")
    finally:
        gpu_session.pack_counts = True
    # the accumulator classes, from the oracle's down-sampled matrices
    a = O.downsample(mats[0], O.column_counts(mats[0]), seed, 300, mode)
    cnt_a = O.column_counts(a)
    ctl_items = A_WIDTH - 1 - 7 * np.arange(len(CUT_HOLDERS))
    assert np.array_equal(cnt_a[ctl_items], CUT_HOLDERS), "the controlled items' cA must survive the down-sampling"
    for d, (m, (st, _)) in enumerate(zip(mats, res)):
        b = a if d == 0 else O.downsample(m, O.column_counts(m), seed, 300, mode)
        rows, users = expected_bins(a, b, m.n_cols, 50)
        assert np.array_equal(st[1:1 + NBINS], rows), f"event {d} (width {m.n_cols}): rows per class {st[1:1 + NBINS]} vs {rows}"
        assert np.array_equal(st[1 + 2 * NBINS:1 + 3 * NBINS], users), f"event {d}: users per class"
        cut = 1 << count_bits(m.n_cols)
        assert cut in CUT_HOLDERS and rows[6] >= sum(h >= cut for h in CUT_HOLDERS), (d, cut, rows)
        assert int(st[1 + 4 * NBINS]) == 0, "LDS accumulator overflow reported"


# ---- relabelling into the widest catalogues: an exact reference without an oracle run at that width -------------------------------
def increasing_map(rng, n, width, anchors):
    """A strictly increasing map of n compact ids into [0, width) through the anchors (0, ids near 2^24 and 2^30, width - 1)."""
    anchors = np.unique([x for x in anchors if 0 <= x < width])
    rest = np.setdiff1d(np.unique(rng.integers(0, width, 2 * n)), anchors)
    ids = np.sort(np.concatenate([anchors, rng.choice(rest, n - anchors.size, replace=False)]))
    assert ids.size == n and np.all(np.diff(ids) > 0)
    return ids


def _anchors(width):
    return [0, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 30) - 1, 1 << 30, width - 1]


def _relabelled(m, n_cols, col_map):
    return O.Csr(m.n_rows, n_cols, m.row_ptr.copy(), col_map[m.col_idx].astype(np.int32))


def _compact_job():
    rng = np.random.default_rng(30)
    a = rand_csr(rng, 20_000, 3_000, 6, zipf_s=1.0)
    b = rand_csr(rng, 20_000, 5_000, 9, zipf_s=0.9)
    cap = int(max(np.diff(a.row_ptr).max(), np.diff(b.row_ptr).max(), O.column_counts(a).max(), O.column_counts(b).max()))
    return a, b, [O.DatasetParams(cap, 10, None)] * 2     # caps >= every row length and column count: the down-sampling is the identity


@pytest.mark.parametrize("width", [(1 << 30) + 1, 0x7FFFFFF0], ids=["2^30+1", "0x7ffffff0"])
def test_relabelled_b_up_to_the_widest_catalogue(gpu_session, width):
    """A compact job, checked against the oracle, with its B columns spread over a catalogue of `width` columns by a strictly increasing map:
    the map keeps (score desc, column asc), so the wide build must give the compact result with mapped ids -- ids exact, LLR bits equal."""
    a, b, params = _compact_job()
    compact, _, _ = compare_with_oracle(gpu_session, [a, b], params, 11)
    want = snapshot(compact)
    fmap = increasing_map(np.random.default_rng(width % 997), b.n_cols, width, _anchors(width))
    bw = _relabelled(b, width, fmap)
    sess = D.DeviceSession(gpu_session.device, gpu_session.lib)
    try:
        got = run_device(sess, [a, bw], params, 11)
        assert np.array_equal(got[1].sampled_col_idx[:bw.nnz].cpu().numpy(), bw.col_idx), "the identity down-sampling changed B"
        got = snapshot(got)
        if width <= (1 << 30) + 1:
            ctx = D.Context(gpu_session.device, gpu_session.lib, 1, 0, 0)
            try:
                assert_same_bits(snapshot(D.cross_occurrence_context(ctx, [to_dev(m, gpu_session.device) for m in (a, bw)], to_params(params), 11)),
                                 got, "context vs session")
            finally:
                ctx.close()
    finally:
        sess.close()
        torch.cuda.empty_cache()
    assert_same_bits(got[:1], want[:1], "A'A")
    rp, ci, llr, st = want[1]
    grp, gci, gllr, gst = got[1]
    assert np.array_equal(grp, rp) and np.array_equal(gci, fmap[ci]) and np.array_equal(gllr, llr), "A'B, mapped back: row_ptr / ids / LLR bits differ"
    assert int(gst[0]) == int(st[0]) and int(gst[1 + 4 * NBINS]) == 0          # (the classes differ: the wide B leaves fewer count bits)
    if width > (1 << 30):
        assert gst[1 + 6] == int((O.column_counts(a) > 1).sum()), "with one count bit every item row of cA > 1 goes to bin 6"


def test_relabelled_a_at_2_25_plus_1_items(gpu_session):
    """The same with A's items spread over 2^25 + 1 (the rows of every indicator matrix and the columns of A'A): rows of unmapped items are
    empty, the others are the compact rows with A'A's ids mapped."""
    a, b, params = _compact_job()
    compact, _, _ = compare_with_oracle(gpu_session, [a, b], params, 12)
    want = snapshot(compact)
    width = (1 << 25) + 1
    fmap = increasing_map(np.random.default_rng(5), a.n_cols, width, _anchors(width))
    aw = _relabelled(a, width, fmap)
    sess = D.DeviceSession(gpu_session.device, gpu_session.lib)
    try:
        got = snapshot(run_device(sess, [aw, b], params, 12))
    finally:
        sess.close()
        torch.cuda.empty_cache()
    for d, ((rp, ci, llr, st), (grp, gci, gllr, gst)) in enumerate(zip(want, got)):
        lens = np.zeros(width, np.int64)
        lens[fmap] = np.diff(rp)
        assert np.array_equal(np.diff(grp), lens), f"event {d}: row lengths"
        assert np.array_equal(gci, fmap[ci] if d == 0 else ci) and np.array_equal(gllr, llr), f"event {d}: ids / LLR bits"
        assert int(gst[0]) == int(st[0]) and int(gst[1 + 4 * NBINS]) == 0
