"""The CONTEXT level of the C ABI on CPU (kernel sources on the test-only host simulator): the host-level entry points
a JNI shim binds, the persistent context behind them, and ONE process driving several (simulated) GPUs -- the shape a
JVM host has -- with the collectives looped back in-process.  Logic only; the parity claims are the -m gpu tests."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import check_indicators, rand_csr, to_dev, to_params
from oracle import c_oracle as O


def P(max_rows=500, k=50, min_llr=None):
    return O.DatasetParams(max_rows, k, min_llr)


def host_level_case(lib):
    """urcco_cooccurrences_idss / urcco_cross_occurrence_downsampled exactly as the Scala host calls them: host CSR in,
    host indicator CSR out, BAD_ARG (never a crash) for inputs that break the stated preconditions."""
    from universal_recommender_amd import _lib
    from universal_recommender_amd import similarity_analysis as SA
    from universal_recommender_amd.indexed_dataset import BiDictionary, IndexedDataset
    rng = np.random.default_rng(12)
    mats = [rand_csr(rng, 3000, 700, 9), rand_csr(rng, 3000, 1500, 14)]
    ids = [IndexedDataset(m.row_ptr, m.col_idx, BiDictionary([f"u{i}" for i in range(m.n_rows)]),
                          BiDictionary([f"i{d}_{i}" for i in range(m.n_cols)])) for d, m in enumerate(mats)]
    ref = O.cross_occurrence_downsampled(mats, [P(30, 10), P(30, 10)], 99)
    for _ in range(2):                                   # the second call reuses the process-wide context and its buffers
        res = SA.cooccurrencesIDSs(ids, randomSeed=99, maxInterestingItemsPerThing=10, maxNumInteractions=30, library=lib)
        for r, o, st in zip(res, ref, SA.last_stats):
            check_indicators((r.row_ptr, r.col_idx, r.values), o)
            assert st.pairs == o.pairs and st.nnz_out == r.nnz and st.nnz_raw > st.nnz_sampled > 0
        assert res[1].rowIDs is ids[0].columnIDs and res[1].columnIDs is ids[1].columnIDs
    assert lib.urcco_shutdown() == 0                     # tears the context down; the next call re-creates it
    res = SA.crossOccurrenceDownsampled([SA.DownsamplableCrossOccurrenceDataset(ids[0], 30, 10, None),
                                         SA.DownsamplableCrossOccurrenceDataset(ids[1], 30, 10, 0.7)], 99, library=lib)
    ref2 = O.cross_occurrence_downsampled(mats, [P(30, 10), P(30, 10, 0.7)], 99)
    for r, o in zip(res, ref2):
        check_indicators((r.row_ptr, r.col_idx, r.values), o)
    # ---- error behaviour: BAD_ARG, not crashes
    u10 = BiDictionary([str(i) for i in range(10)])
    bad_rows = IndexedDataset(np.zeros(11, np.int64), np.zeros(0, np.int32), u10, BiDictionary(["x"]))
    with pytest.raises(_lib.UrccoError) as ei:
        SA.cooccurrencesIDSs([ids[0], bad_rows], library=lib)
    assert ei.value.status == _lib.BAD_ARG
    with pytest.raises(_lib.UrccoError):
        SA.cooccurrencesIDSs(ids, maxInterestingItemsPerThing=0, library=lib)
    cols4 = BiDictionary(["a", "b", "c", "d"])
    rp = np.array([0, 2, 4] + [4] * 8, np.int64)
    for ci, what in [([0, 7, 1, 2], "column out of range"), ([0, -1, 1, 2], "negative column"), ([1, 0, 1, 2], "not increasing"),
                     ([1, 1, 1, 2], "duplicate column")]:
        bad = IndexedDataset(rp, np.array(ci, np.int32), u10, cols4)
        with pytest.raises(_lib.UrccoError) as ei:
            SA.cooccurrencesIDSs([bad], library=lib)
        assert ei.value.status == _lib.BAD_ARG, what
    bad = IndexedDataset(np.array([0, 3, 2] + [4] * 8, np.int64), np.array([0, 1, 2, 3], np.int32), u10, cols4)
    with pytest.raises(_lib.UrccoError) as ei:
        SA.cooccurrencesIDSs([bad], library=lib)
    assert ei.value.status == _lib.BAD_ARG
    good = IndexedDataset(rp, np.array([0, 3, 1, 2], np.int32), u10, cols4)
    assert SA.cooccurrencesIDSs([good], library=lib)[0].nrow == 4
    lib.urcco_shutdown()


def test_host_level_entry_points(sim_lib):
    host_level_case(sim_lib)


def context_reuse_case(lib, device):
    """One context, several builds of different shapes (its buffers grow, then are reused): each equals the one-session
    stage-by-stage driver bit for bit, in stream-per-event and single-stream mode."""
    from universal_recommender_amd import _lib
    from universal_recommender_amd.device import Context, DeviceSession, cross_occurrence_context, cross_occurrence_device
    rng = np.random.default_rng(41)
    cases = [([rand_csr(rng, 3000, 400, 10, zipf_s=1.1), rand_csr(rng, 3000, 600, 16), rand_csr(rng, 3000, 50, 2)], [P(80, 20), P(80, 20), P(500, 50)]),
             ([rand_csr(rng, 9000, 900, 12), rand_csr(rng, 9000, 30, 3)], [P(40, 10), P(40, 5, 0.2)]),
             ([rand_csr(rng, 500, 40, 5)], [P(20, 7)])]
    sess = DeviceSession(device, lib)
    ctx = Context(device, lib)
    try:
        for flags, dbg in ((0, 0), (_lib.FLAG_SINGLE_STREAM, 0), (0, _lib.DBG_UNPACKED_COUNTS)):   # B' without the counts aboard (one count gather per candidate)
            ctx.set_flags(flags)
            ctx.set_debug(dbg)
            for mats, ps in cases:
                ref = cross_occurrence_device(sess, [to_dev(m, device) for m in mats], to_params(ps), 17)
                sess.synchronize()
                for _ in range(2):
                    out = cross_occurrence_context(ctx, [to_dev(m, device) for m in mats], to_params(ps), 17)
                    for a, b in zip(out, ref):
                        for x, y in zip(a.to_host(), b.to_host()):
                            assert np.array_equal(x, y)
                        assert torch.equal(a.stats[:1].cpu(), b.stats[:1].cpu())
                        assert torch.equal(a.sampled_row_ptr.cpu(), b.sampled_row_ptr.cpu())
    finally:
        ctx.close()
        sess.close()


def back_to_back_builds_case(lib, device, n_users):
    """Builds enqueued back to back WITHOUT waiting in between (what bench.py's timed region does): the next build's primary
    chain runs on stream 0 while the previous build's A'B_d still read the primary's CSC and counts on their own streams,
    so those live in alternating buffer sets.  The secondaries are made much heavier than the primary so that their
    streams lag; shapes alternate so that a clobbered CSC would index out of range.  The last build must equal the
    one-session driver bit for bit."""
    from universal_recommender_amd.device import Context, DeviceSession, cross_occurrence_context, cross_occurrence_device
    rng = np.random.default_rng(43)
    x = ([rand_csr(rng, n_users, 300, 4), rand_csr(rng, n_users, 2500, 40, zipf_s=1.05), rand_csr(rng, n_users, 1200, 25)], [P(60, 20), P(60, 30), P(60, 30)])
    y = ([rand_csr(rng, n_users // 3, 5000, 9), rand_csr(rng, n_users // 3, 700, 30)], [P(100, 10), P(100, 10)])
    sess = DeviceSession(device, lib)
    ctx = Context(device, lib)
    try:
        refs = []
        for mats, ps in (x, y):
            refs.append([r.to_host() for r in cross_occurrence_device(sess, [to_dev(m, device) for m in mats], to_params(ps), 23)])
            sess.synchronize()
        dev = [([to_dev(m, device) for m in mats], to_params(ps)) for mats, ps in (x, y)]
        for last in (0, 1):
            for i in range(7):
                mats, ps = dev[(i + last) % 2]
                ctx.build([[m] for m in mats], ps, 23)           # enqueue only
            out = [r[0] for r in ctx.results()]                    # waits for the last build
            assert len(out) == len(refs[last])
            for a, b in zip(out, refs[last]):
                for u, v in zip(a.to_host(), b):
                    assert np.array_equal(u, v)
    finally:
        ctx.close()
        sess.close()


def test_back_to_back_builds(sim_lib):
    back_to_back_builds_case(sim_lib, torch.device("cpu"), 3000)


def test_context_reuse_and_stream_modes(sim_lib):
    context_reuse_case(sim_lib, torch.device("cpu"))


@pytest.mark.parametrize("n_gpus,primary", [(2, "fragments"), (3, "fragments"), (5, "fragments"), (2, "gathered"), (3, "plain rows")])
def test_one_process_drives_several_gpus(sim_lib, n_gpus, primary, monkeypatch):
    """n_gpus ranks in ONE process (what the JVM host does; here simulated devices, collectives looped back in-process
    through the urcco_collectives callbacks): the device-resident build on user-range shards and the host-level build
    (the library shards the users itself, balances the item ranges by work, concatenates the slices) both equal the
    single-GPU oracle."""
    from universal_recommender_amd import _lib, sharded
    from universal_recommender_amd.device import Context
    monkeypatch.setenv("HIPSIM_DEVICE_COUNT", str(n_gpus))
    rng = np.random.default_rng(5)
    n_users = 2500
    mats = [rand_csr(rng, n_users, 300, 9, zipf_s=1.2), rand_csr(rng, n_users, 700, 14), rand_csr(rng, n_users, 900, 6),
            rand_csr(rng, n_users, 40, 4), rand_csr(rng, n_users, 11, 2, empty_frac=0.3)]
    params = [P(30, 10), P(40, 12), P(25, 50), P(500, 8), P(500, 50, 0.1)]
    ref = O.cross_occurrence_downsampled(mats, params, 2024)
    coll = sharded.TorchCollectives(n_gpus, list(range(n_gpus)))
    ctx = Context(torch.device("cpu"), sim_lib, n_gpus=n_gpus, collectives=coll)
    if primary == "gathered":
        ctx.set_debug(_lib.DBG_GATHERED_PRIMARY)       # A/B path: the primary's CSC from a pass over the whole gathered A' instead of fragments
    if primary == "plain rows":
        ctx.set_debug(_lib.DBG_UNPACKED_COUNTS)    # the rows travel as plain column indices, the row kernels gather the counts (the form of rounds 1-5)
    try:
        assert ctx.n_local == n_gpus
        cuts = [n_users * g // n_gpus for g in range(n_gpus + 1)]
        cuts[1] = 100                                                     # uneven shards
        shards = [[to_dev(O.Csr(hi - lo, m.n_cols, m.row_ptr[lo:hi + 1] - m.row_ptr[lo], m.col_idx[m.row_ptr[lo]:m.row_ptr[hi]]), "cpu")
                   for lo, hi in zip(cuts, cuts[1:])] for m in mats]
        ctx.build(shards, to_params(params), 2024, n_users, cuts[:-1])
        res = ctx.results()
        for d, r in enumerate(ref):
            parts = [ind.to_host() for ind in res[d]]
            assert res[d][0].item_lo == 0 and res[d][-1].item_hi == mats[0].n_cols
            assert all(a.item_hi == b.item_lo for a, b in zip(res[d], res[d][1:]))
            lens = np.concatenate([np.diff(p[0]) for p in parts])
            rp = np.zeros(lens.size + 1, np.int64)
            np.cumsum(lens, out=rp[1:])
            check_indicators((rp, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])), r, exact_ids=True)
            assert sum(int(ind.stats[0]) for ind in res[d]) == r.pairs
            full = O.downsample(mats[d], O.column_counts(mats[d]), 2024, params[d].max_elements_per_row)
            for ind in res[d]:
                #  the size of the WHOLE down-sampled matrix comes from the library's own total, whatever this GPU holds of it
                assert ind.sampled_nnz_total == full.nnz and ind.nnz_sampled_global() == full.nnz
                if primary == "gathered":                                 # every GPU holds the whole down-sampled B
                    assert np.array_equal(ind.sampled_row_ptr.numpy(), full.row_ptr)
                    assert np.array_equal(ind.sampled_col_idx.numpy()[:full.nnz], full.col_idx)
                else:       # row-filtered exchange: a GPU holds the rows of the users its item range touches -- whole -- and empty rows for the others
                    rp_g, ci_g = ind.sampled_row_ptr.numpy(), ind.sampled_col_idx.numpy()
                    lens_g, lens_f = np.diff(rp_g), np.diff(full.row_ptr)
                    assert np.all((lens_g == lens_f) | (lens_g == 0))
                    held = np.nonzero(lens_g)[0]
                    assert np.array_equal(ci_g[:rp_g[-1]], np.concatenate([full.col_idx[full.row_ptr[u]:full.row_ptr[u + 1]] for u in held] + [np.zeros(0, np.int32)]))
                    if n_gpus >= 3 and d == 1:
                        assert 0 < held.size < np.count_nonzero(lens_f), "the filter must drop some rows and keep some"
        # host level on the same context
        n = len(mats)
        arr = (_lib.Dataset * n)()
        for d, (m, p) in enumerate(zip(mats, params)):
            arr[d].matrix.n_rows, arr[d].matrix.n_cols = m.n_rows, m.n_cols
            arr[d].matrix.row_ptr, arr[d].matrix.col_idx = m.row_ptr.ctypes.data, m.col_idx.ctypes.data
            arr[d].max_elements_per_row, arr[d].max_interesting_elements = p.max_elements_per_row, p.max_interesting_elements
            arr[d].has_min_llr, arr[d].min_llr = int(p.min_llr is not None), float(p.min_llr or 0.0)
        out = (_lib.Indicators * n)()
        stats = (_lib.DatasetStats * n)()
        _lib.check(sim_lib.urcco_context_cross_occurrence(ctx.handle, arr, n, 2024, out, stats), sim_lib)
        for d, r in enumerate(ref):
            o = out[d]
            nnz = int(o.nnz)
            got = (np.ctypeslib.as_array(o.row_ptr, shape=(o.n_rows + 1,)).copy(), np.ctypeslib.as_array(o.col_idx, shape=(max(nnz, 1),))[:nnz].copy(),
                   np.ctypeslib.as_array(o.llr, shape=(max(nnz, 1),))[:nnz].copy())
            check_indicators(got, r, exact_ids=True)
            assert stats[d].pairs == r.pairs and stats[d].nnz_out == nnz and stats[d].nnz_raw == mats[d].nnz
        sim_lib.urcco_free_indicators(out, n)
        assert coll.error is None
        # what travelled
        a2a = [e for e in coll.log if e[0] == "aa"]
        if primary in ("fragments", "plain rows"):
            # per build and rank: the primary's CSC as fragments (16-bit column lengths, then entries) + per event type the row-filtered
            # exchange (masked row lengths to every destination, then the rows a destination may see)
            assert len(a2a) == 2 * n_gpus * (2 + 2 * len(mats))
            assert any(e[1] == 0 and sum(e[2]) == 2 * mats[0].n_cols for e in a2a)   # rank 0 sends every column's length once, as uint16
            assert a2a[0] == ("aa", 0, (2 * 100,) * n_gpus)                          # rank 0's 100 masked row lengths to every rank, as uint16
            sampled = O.downsample(mats[0], O.column_counts(mats[0]), 2024, params[0].max_elements_per_row)
            cols0 = [sum(e[2]) for e in a2a[n_gpus:2 * n_gpus]]                      # A' rows as packed per destination (first event type, first build)
            assert 4 * sampled.nnz <= sum(cols0) + 4 * int((np.diff(sampled.row_ptr) == 0).sum()) and sum(cols0) <= n_gpus * 4 * sampled.nnz
            if n_gpus >= 3:
                assert sum(cols0) < n_gpus * 4 * sampled.nnz, "not every row goes to every rank"
            assert not any(e[0] == "ag" and e[2] == 4 * sampled.nnz for e in coll.log)   # no all-gather of whole matrices any more
        else:
            assert not a2a
            assert any(e[0] == "ag" and e[2] == 2 * 100 for e in coll.log)     # rank 0's 100 row lengths of one event type, as uint16
    finally:
        ctx.close()


def test_exchange_falls_back_to_32_bit_lengths(sim_lib, monkeypatch):
    """Column lengths of a shard's CSC and row lengths of a shard travel as uint16 unless one does not fit: a primary column held
    by 70 000 users of one shard switches that build's fragments to int32 lengths, a secondary user with 66 000 items switches that
    event type's row lengths to int32 (decided from the records every rank publishes, so all ranks agree) -- and the result is
    still the oracle's."""
    from universal_recommender_amd import sharded
    from universal_recommender_amd.device import Context
    n_gpus = 2
    monkeypatch.setenv("HIPSIM_DEVICE_COUNT", str(n_gpus))
    rng = np.random.default_rng(8)
    n_users, n_a, n_b = 80_000, 300, 66_500
    extra = rng.integers(1, n_a, (n_users, 2))
    rows = [np.unique(np.concatenate([[0] if u < 70_000 else [], extra[u]])).astype(np.int32) for u in range(n_users)]
    rp = np.zeros(n_users + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    a = O.Csr(n_users, n_a, rp, np.concatenate(rows).astype(np.int32))
    brows = [np.unique(rng.integers(0, n_b, 2)).astype(np.int32) for _ in range(n_users)]
    brows[75_000] = np.arange(66_000, dtype=np.int32)                    # one very long row in the second shard
    rp = np.zeros(n_users + 1, np.int64)
    np.cumsum([len(r) for r in brows], out=rp[1:])
    b = O.Csr(n_users, n_b, rp, np.concatenate(brows).astype(np.int32))
    mats, params = [a, b], [P(100_000, 5), P(100_000, 5)]
    ref = O.cross_occurrence_downsampled(mats, params, 11)
    coll = sharded.TorchCollectives(n_gpus, list(range(n_gpus)))
    ctx = Context(torch.device("cpu"), sim_lib, n_gpus=n_gpus, collectives=coll)
    try:
        cuts = [0, 72_000, n_users]
        shards = [[to_dev(O.Csr(hi - lo, m.n_cols, m.row_ptr[lo:hi + 1] - m.row_ptr[lo], m.col_idx[m.row_ptr[lo]:m.row_ptr[hi]]), "cpu")
                   for lo, hi in zip(cuts, cuts[1:])] for m in mats]
        ctx.build(shards, to_params(params), 11, n_users, cuts[:-1])
        res = ctx.results()
        for d, r in enumerate(ref):
            parts = [ind.to_host() for ind in res[d]]
            ln = np.concatenate([np.diff(p[0]) for p in parts])
            full_rp = np.zeros(ln.size + 1, np.int64)
            np.cumsum(ln, out=full_rp[1:])
            check_indicators((full_rp, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])), r, exact_ids=True)
        assert coll.error is None
        a2a = [e for e in coll.log if e[0] == "aa"]
        assert any(e[1] == 0 and sum(e[2]) == 4 * n_a for e in a2a)        # the fragments' column lengths as int32
        assert not any(e[1] == 0 and sum(e[2]) == 2 * n_a for e in a2a)
        assert any(e[1] == 0 and e[2] == (2 * 72_000,) * n_gpus for e in a2a)   # the primary's (masked) row lengths as uint16 ...
        assert any(e[1] == 0 and e[2] == (4 * 72_000,) * n_gpus for e in a2a)   # ... the secondary's as int32
    finally:
        ctx.close()


def unordered_rows_case(lib, device):
    """URCCO_FLAG_UNORDERED_ROWS: every row holds exactly the oracle's top-k set (ids and scores), in arbitrary order --
    all accumulator classes, k boundary with ties, minLLR."""
    from universal_recommender_amd import _lib
    from universal_recommender_amd.device import Context, cross_occurrence_context
    from helpers import sort_rows
    import test_sim_kernel_logic as logic
    rng = np.random.default_rng(2)
    cases = [([rand_csr(rng, 4000, 20000, 12, zipf_s=1.2), rand_csr(rng, 4000, 30000, 25, zipf_s=1.1)], [P(10000, 50), P(10000, 20)]),
             ([rand_csr(rng, 300, 80, 6), rand_csr(rng, 300, 40, 9), rand_csr(rng, 300, 7, 2)], [P(20, 5), P(30, 7, 0.5), P(500, 3)]),
             ([logic._tied_block(13, 150, 2, np.arange(150))] * 2, [P(100000, 20), P(100000, 20)]),
             ([rand_csr(rng, 1500, 40, 6, zipf_s=1.5), rand_csr(rng, 1500, 17000, 40, zipf_s=0.3)], [P(100000, 10), P(100000, 60)])]
    ctx = Context(device, lib, flags=_lib.FLAG_UNORDERED_ROWS)
    try:
        for mats, ps in cases:
            ref = O.cross_occurrence_downsampled(mats, ps, 5)
            out = cross_occurrence_context(ctx, [to_dev(m, device) for m in mats], to_params(ps), 5)
            for o, r in zip(out, ref):
                assert int(o.stats[0]) == r.pairs
                check_indicators(sort_rows(o.to_host()), r)
    finally:
        ctx.close()


def test_unordered_rows_flag(sim_lib):
    unordered_rows_case(sim_lib, torch.device("cpu"))


def fused_expand_case(lib, device):
    """The fused expand preparation of the secondaries (one interleaved (start, length) gather per CSC entry of A' for every
    secondary at once) against the per-event form (debug 4096) and the one-session driver, bit for bit: 2, 5 and 8 secondaries
    (the most one fused pass takes), 9 (falls back to the per-event form), an EMPTY secondary, stream-per-event and
    single-stream mode, twice per shape (the buffers are reused)."""
    from universal_recommender_amd import _lib
    from universal_recommender_amd.device import Context, DeviceSession, cross_occurrence_context, cross_occurrence_device
    rng = np.random.default_rng(47)
    sess = DeviceSession(device, lib)
    try:
        # (the last shape: > 32768 CSC entries of A' -- the tiled scans, whose tile sums the fused pass leaves behind, over a partial last tile)
        for n_users, n_sec in ((1500, 2), (1500, 5), (1500, 8), (1500, 9), (9000, 3)):
            empty = O.Csr(n_users, 9, np.zeros(n_users + 1, np.int64), np.zeros(0, np.int32))
            mats = [rand_csr(rng, n_users, 300, 5 if n_users < 9000 else 7, zipf_s=1.1)] + [rand_csr(rng, n_users, 40 + 37 * d, 3 + d, empty_frac=0.1 * (d % 3)) for d in range(n_sec)]
            if n_sec == 5:
                mats[3] = empty
            if n_users >= 9000:
                assert mats[0].row_ptr[-1] > 40000
            ps = [P(30, 10)] + [P(25 + d, 6 + d, 0.1 if d == 1 else None) for d in range(n_sec)]
            ref = [r.to_host() for r in cross_occurrence_device(sess, [to_dev(m, device) for m in mats], to_params(ps), 5)]
            sess.synchronize()
            for flags in (0, _lib.FLAG_SINGLE_STREAM):
                for debug in (0, _lib.DBG_UNFUSED_EXPAND):
                    ctx = Context(device, lib, flags=flags)
                    try:
                        ctx.set_debug(debug)
                        for _ in range(2):
                            out = cross_occurrence_context(ctx, [to_dev(m, device) for m in mats], to_params(ps), 5)
                            assert len(out) == len(ref)
                            for a, b in zip(out, ref):
                                for x, y in zip(a.to_host(), b):
                                    assert np.array_equal(x, y)
                    finally:
                        ctx.close()
    finally:
        sess.close()


def test_fused_expand_of_the_secondaries(sim_lib):
    fused_expand_case(sim_lib, torch.device("cpu"))


def test_stage_finish_protocol(sim_lib):
    """urcco_context_stage / _finish: finish without stage, a second stage before finish and a mismatching finish count are
    BAD_ARG; a staged build that nobody finishes is abandoned cleanly by urcco_shutdown / context destruction; out[] of a
    failing call is zeroed (the caller's garbage is never freed)."""
    import ctypes as C
    from universal_recommender_amd import _lib
    lib = sim_lib
    rng = np.random.default_rng(53)
    mats = [rand_csr(rng, 400, 60, 5), rand_csr(rng, 400, 30, 4), rand_csr(rng, 400, 12, 2)]
    n = len(mats)
    arr = (_lib.Dataset * n)()
    for d, m in enumerate(mats):
        arr[d].matrix.n_rows, arr[d].matrix.n_cols = m.n_rows, m.n_cols
        arr[d].matrix.row_ptr, arr[d].matrix.col_idx = m.row_ptr.ctypes.data, m.col_idx.ctypes.data
        arr[d].max_elements_per_row, arr[d].max_interesting_elements = 500, 50
    opts = _lib.Options(device=0, row_rate_mode=0, n_gpus=1)
    out = (_lib.Indicators * n)()
    lib.urcco_shutdown()
    assert lib.urcco_cross_occurrence_finish(out, n, None) == _lib.BAD_ARG          # nothing staged
    assert lib.urcco_cross_occurrence_stage(arr, n, 3, C.byref(opts)) == _lib.OK
    assert lib.urcco_cross_occurrence_stage(arr, n, 3, C.byref(opts)) == _lib.BAD_ARG   # the previous one is not finished
    # a finish that cannot take what was staged DISCARDS it and frees the default context (the early return used to leave it
    # occupied for good); so does urcco_cross_occurrence_cancel
    assert lib.urcco_cross_occurrence_finish(out, n - 1, None) == _lib.BAD_ARG
    assert b"discarded" in lib.urcco_last_error()
    assert lib.urcco_cross_occurrence_finish(out, n, None) == _lib.BAD_ARG             # nothing staged any more
    assert lib.urcco_cross_occurrence_stage(arr, n, 3, C.byref(opts)) == _lib.OK
    assert lib.urcco_cross_occurrence_cancel() == _lib.OK
    assert lib.urcco_cross_occurrence_cancel() == _lib.OK                               # nothing staged: a no-op
    assert lib.urcco_cross_occurrence_finish(out, n, None) == _lib.BAD_ARG
    # a thread that staged and walked away: another thread's stage gives up after URCCO_STAGE_WAIT_S instead of hanging for ever
    import threading
    assert lib.urcco_cross_occurrence_stage(arr, n, 3, C.byref(opts)) == _lib.OK
    os.environ["URCCO_STAGE_WAIT_S"] = "1"
    got = []
    try:
        t = threading.Thread(target=lambda: got.append(lib.urcco_cross_occurrence_stage(arr, n, 3, C.byref(opts))))
        t.start()
        t.join(30)
    finally:
        del os.environ["URCCO_STAGE_WAIT_S"]
    assert got == [_lib.BUSY], got                                                     # a status of its own, not INTERNAL
    # ... and that thread cannot discard the owner's build: _cancel from a non-owner is BUSY and leaves it staged (the owner's _finish works)
    got = []
    t = threading.Thread(target=lambda: got.append(lib.urcco_cross_occurrence_cancel()))
    t.start()
    t.join(30)
    assert got == [_lib.BUSY], got
    assert lib.urcco_cross_occurrence_finish(out, n, None) == _lib.OK
    ref = O.cross_occurrence_downsampled(mats, [P()] * n, 3)
    for d, r in enumerate(ref):
        o = out[d]
        nnz = int(o.nnz)
        check_indicators((np.ctypeslib.as_array(o.row_ptr, shape=(o.n_rows + 1,)).copy(), np.ctypeslib.as_array(o.col_idx, shape=(max(nnz, 1),))[:nnz].copy(),
                          np.ctypeslib.as_array(o.llr, shape=(max(nnz, 1),))[:nnz].copy()), r)
    lib.urcco_free_indicators(out, n)
    # an owner that is gone: only _cancel_any frees the context for the others; the owner's late _finish then finds nothing staged
    t = threading.Thread(target=lambda: got.append(lib.urcco_cross_occurrence_stage(arr, n, 3, C.byref(opts))))
    t.start()
    t.join(30)
    assert got[-1] == _lib.OK
    assert lib.urcco_cross_occurrence_cancel() == _lib.BUSY
    assert lib.urcco_cross_occurrence_cancel_any() == _lib.OK
    assert lib.urcco_cross_occurrence_finish(out, n, None) == _lib.BAD_ARG
    assert lib.urcco_cross_occurrence_stage(arr, n, 3, C.byref(opts)) == _lib.OK
    assert lib.urcco_shutdown() == 0                                                  # abandons the staged build
    assert lib.urcco_cross_occurrence_finish(out, n, None) == _lib.BAD_ARG
    # a failing one-shot call leaves out[] zeroed even if the caller handed in garbage pointers
    junk = (_lib.Indicators * n)()
    for d in range(n):
        junk[d].nnz = 7
        junk[d].row_ptr = C.cast(C.c_void_p(0xdead0000), C.POINTER(C.c_int64))
    bad_opts = _lib.Options(device=99, row_rate_mode=0, n_gpus=1)
    assert lib.urcco_cross_occurrence_downsampled(arr, n, 3, C.byref(bad_opts), junk, None) == _lib.BAD_ARG
    assert all(not junk[d].row_ptr and junk[d].nnz == 0 for d in range(n))
    lib.urcco_shutdown()


def test_one_shot_calls_from_two_threads_serialise(sim_lib):
    """The one-shot entry points share one process-wide context; a build occupies it from its stage to its finish (the
    lock was dropped between the two halves, so a second thread's stage failed -- or, with different options, destroyed the context
    under the first thread's pending build).  Two threads now call urcco_cross_occurrence_downsampled at once, with DIFFERENT flags
    (each call re-creates the default context): both must succeed and equal the oracle."""
    import ctypes as C
    import threading
    from universal_recommender_amd import _lib
    lib = sim_lib
    lib.urcco_shutdown()
    rng = np.random.default_rng(77)
    jobs = []
    for t in range(2):
        mats = [rand_csr(rng, 3000, 400, 8, zipf_s=1.1), rand_csr(rng, 3000, 250, 12)]
        jobs.append((mats, 11 + t, _lib.FLAG_UNORDERED_ROWS if t else 0))
    results, errors = {}, {}

    def run(t):
        mats, seed, flags = jobs[t]
        n = len(mats)
        arr = (_lib.Dataset * n)()
        for d, m in enumerate(mats):
            arr[d].matrix.n_rows, arr[d].matrix.n_cols = m.n_rows, m.n_cols
            arr[d].matrix.row_ptr, arr[d].matrix.col_idx = m.row_ptr.ctypes.data, m.col_idx.ctypes.data
            arr[d].max_elements_per_row, arr[d].max_interesting_elements = 500, 50
        opts = _lib.Options(device=0, row_rate_mode=0, n_gpus=1, flags=flags)
        for rep in range(3):
            out = (_lib.Indicators * n)()
            st = lib.urcco_cross_occurrence_downsampled(arr, n, seed, C.byref(opts), out, None)
            if st != _lib.OK:
                errors[t] = (st, lib.urcco_last_error())
                return
            got = []
            for d in range(n):
                o = out[d]
                nnz = int(o.nnz)
                got.append((np.ctypeslib.as_array(o.row_ptr, shape=(o.n_rows + 1,)).copy(), np.ctypeslib.as_array(o.col_idx, shape=(max(nnz, 1),))[:nnz].copy(),
                            np.ctypeslib.as_array(o.llr, shape=(max(nnz, 1),))[:nnz].copy()))
            lib.urcco_free_indicators(out, n)
            results[t] = got

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=300)
    assert not any(th.is_alive() for th in threads), "a one-shot call never returned"
    assert not errors, errors
    from helpers import sort_rows
    for t, (mats, seed, flags) in enumerate(jobs):
        ref = O.cross_occurrence_downsampled(mats, [P()] * len(mats), seed)
        for got, r in zip(results[t], ref):
            check_indicators(sort_rows(got) if flags else got, r)
    lib.urcco_shutdown()


def test_row_filtered_exchange_volume_at_8_ranks(sim_lib, monkeypatch):
    """at 8 ranks a rank must receive clearly less than the all-gather of every down-sampled matrix.  BASELINE config 4's
    generator at 1/100 (100K users, 5 event types), 8 simulated GPUs in one process, the collectives' log as the wire: with the
    row-filtered exchange (default) every rank receives <= 0.6 x what the all-gather form (debug 16384) delivers to it -- B' rows travel
    only to the ranks whose item range their user touches -- and both builds equal the oracle."""
    from universal_recommender_amd import _lib, sharded, synth
    from universal_recommender_amd.device import Context
    W = 8
    monkeypatch.setenv("HIPSIM_DEVICE_COUNT", str(W))
    cfg = synth.config4(0.01)
    data = synth.generate(cfg)
    mats = [O.Csr(cfg.n_users, nc, rp, ci) for (_, nc, rp, ci) in data]
    params = [P()] * len(mats)
    ref = O.cross_occurrence_downsampled(mats, params, 7)
    cuts = [cfg.n_users * g // W for g in range(W + 1)]
    shards = [[to_dev(O.Csr(hi - lo, m.n_cols, m.row_ptr[lo:hi + 1] - m.row_ptr[lo], m.col_idx[m.row_ptr[lo]:m.row_ptr[hi]]), "cpu")
               for lo, hi in zip(cuts, cuts[1:])] for m in mats]
    received = {}
    for mode, debug in (("filtered", 0), ("all-gather", _lib.DBG_UNFILTERED_EXCHANGE)):
        coll = sharded.TorchCollectives(W, list(range(W)))
        ctx = Context(torch.device("cpu"), sim_lib, n_gpus=W, collectives=coll)
        try:
            ctx.set_debug(debug)
            ctx.build(shards, to_params(params), 7, cfg.n_users, cuts[:-1])
            res = ctx.results()
            for d, r in enumerate(ref):
                parts = [ind.to_host() for ind in res[d]]
                lens = np.concatenate([np.diff(p[0]) for p in parts])
                rp = np.zeros(lens.size + 1, np.int64)
                np.cumsum(lens, out=rp[1:])
                check_indicators((rp, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])), r)
                assert sum(int(ind.stats[0]) for ind in res[d]) == r.pairs
            assert coll.error is None
            recv = np.zeros(W, np.int64)
            for e in coll.log:
                if e[0] == "aa":                      # (kind, sender, bytes to every destination)
                    for q, b in enumerate(e[2]):
                        if q != e[1]:
                            recv[q] += b
                elif e[0] == "ag":                    # (kind, sender, bytes contributed): every other rank receives them
                    recv += e[2]
                    recv[e[1]] -= e[2]
            received[mode] = recv
        finally:
            ctx.close()
    ratio = received["filtered"] / received["all-gather"]
    assert np.all(ratio <= 0.6), (ratio, received)
    assert np.all(ratio >= 0.15), ratio       # sanity: it still receives the rows it multiplies with


def test_emulated_ranks_on_one_device(sim_lib):
    """URCCO_FLAG_EMULATE_RANKS (bench.py --emulate-ranks): W ranks of a job on ONE device and one stream, collectives looped back through
    views on the library's buffers.  The build is the real W-rank build -- fragments, row-filtered exchange, fused expand, work-balanced
    ranges -- so every rank's rows must equal the oracle, and every rank reports its own stage timings."""
    from universal_recommender_amd import _lib, sharded, synth
    from universal_recommender_amd.device import Context
    W = 4
    cfg = synth.config4(0.004)
    data = synth.generate(cfg)
    mats = [O.Csr(cfg.n_users, nc, rp, ci) for (_, nc, rp, ci) in data]
    params = [P(60, 12)] * len(mats)
    ref = O.cross_occurrence_downsampled(mats, params, 11)
    cuts = [cfg.n_users * g // W for g in range(W + 1)]
    shards = [[to_dev(O.Csr(hi - lo, m.n_cols, m.row_ptr[lo:hi + 1] - m.row_ptr[lo], m.col_idx[m.row_ptr[lo]:m.row_ptr[hi]]), "cpu")
               for lo, hi in zip(cuts, cuts[1:])] for m in mats]
    with pytest.raises(_lib.UrccoError):      # RCCL cannot put two ranks on one device: the flag needs caller-supplied collectives
        Context(torch.device("cpu"), sim_lib, n_gpus=W, flags=_lib.FLAG_EMULATE_RANKS)
    coll = sharded.DeviceLoopbackCollectives(W, "cpu")
    ctx = Context(torch.device("cpu"), sim_lib, n_gpus=W, flags=_lib.FLAG_EMULATE_RANKS, collectives=coll)
    try:
        assert ctx.n_local == W
        ctx.set_timing(True)
        for _ in range(2):                     # the second build reuses every buffer
            ctx.build(shards, to_params(params), 11, cfg.n_users, cuts[:-1])
            res = ctx.results()
            assert coll.error is None
            for d, r in enumerate(ref):
                parts = [ind.to_host() for ind in res[d]]
                assert res[d][0].item_lo == 0 and res[d][-1].item_hi == mats[0].n_cols
                assert all(a.item_hi == b.item_lo for a, b in zip(res[d], res[d][1:]))
                lens = np.concatenate([np.diff(p[0]) for p in parts])
                rp = np.zeros(lens.size + 1, np.int64)
                np.cumsum(lens, out=rp[1:])
                check_indicators((rp, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])), r)
                assert sum(int(ind.stats[0]) for ind in res[d]) == r.pairs
                assert all(ind.sampled_nnz_total == O.downsample(mats[d], O.column_counts(mats[d]), 11, 60).nnz for ind in res[d])
        per_rank = [ctx.get_timings_gpu(g) for g in range(W)]
        total = ctx.get_timings()
        for name in ("column_counts", "downsample_flags", "transpose", "exchange", "cco_rows_micro", "compact_indicators"):
            assert all(t[name][1] > 0 for t in per_rank), name                      # every rank ran the stage ...
            assert sum(t[name][1] for t in per_rank) == total[name][1], name        # ... and the per-rank views add up to the context's
        assert all(b > 0 for b in coll.bytes_received)
    finally:
        ctx.close()


def test_eight_ranks_and_the_exchange_route_on_config5_skew_every_row(sim_session):
    """The CPU-suite twin of tests/test_gpu_scale.py::test_full_config4_every_row / test_full_config5_every_row: BASELINE
    config 5's generator (hot head, heavy users; 1/250 of the users, item spaces 1/50) built three ways -- one rank, one rank through the
    exchange route (URCCO_FLAG_FORCE_EXCHANGE), eight emulated ranks -- and every row of every build checked against ONE oracle pass,
    the rows a rank holds of the down-sampled matrices included."""
    from helpers import RanksOfAJob, compare_with_oracle_large, shard_rows
    from universal_recommender_amd import _lib, sharded, synth
    from universal_recommender_amd import device as D
    cfg = synth.config5(0.004, item_scale=0.02)
    mats = [O.Csr(cfg.n_users, nc, rp, ci) for (_, nc, rp, ci) in synth.generate(cfg)]
    assert max(int(np.diff(m.row_ptr).max()) for m in mats) > 60
    params = [P(60, 12)] * len(mats)
    dev_mats = [to_dev(m, "cpu") for m in mats]
    W = 8
    shards, cuts = shard_rows(dev_mats, W)
    coll8 = sharded.DeviceLoopbackCollectives(W, "cpu")
    ctx8 = D.Context(torch.device("cpu"), sim_session.lib, W, _lib.FLAG_EMULATE_RANKS, collectives=coll8)
    coll1 = sharded.TorchCollectives(1, [0])
    ctx_x = D.Context(torch.device("cpu"), sim_session.lib, 1, _lib.FLAG_FORCE_EXCHANGE, collectives=coll1)
    try:
        ctx8.build(shards, to_params(params), 77, cfg.n_users, cuts[:-1])
        res8 = ctx8.results()
        out_x = D.cross_occurrence_context(ctx_x, dev_mats, to_params(params), 77)
        assert coll8.error is None and coll1.error is None
        _, res = compare_with_oracle_large(sim_session, mats, params, 77, dev_mats=dev_mats, via_context=True, threads=4,
                                           also=[("8 emulated ranks", [RanksOfAJob(row) for row in res8]), ("exchange route", out_x)])
        work = np.array([sum(int(res8[d][g].stats[0]) for d in range(len(mats))) for g in range(W)], np.float64)
        assert work.max() / work.mean() < 1.25, work      # work-balanced item ranges (a small job: coarse)
        assert sum(int(st[0]) for st, _ in res) == int(work.sum())
    finally:
        res8 = out_x = None
        ctx8.close()
        ctx_x.close()
