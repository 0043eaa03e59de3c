"""The k11 = 1 prefilter of the packed row kernels (csrc/cco_rows.hip) on the host simulator: every case is compared with the oracle AND, bit for bit
(row lengths, ids in order, LLR bits), with the same build run with the prefilter switched off (debug bit NO_PREFILTER); the scored-candidate count
(debug bit COUNT_SCORED, stats[30] while stage timing is on) is compared with a plain-numpy model of the rule whose limits are re-derived from the
definition of the monotone-limit table through urcco_dev_llr -- the table itself is not readable through the C ABI, its consequences are."""
import numpy as np
import pytest

from helpers import compare_with_oracle, rand_csr, run_device
from oracle import c_oracle as O
from prefilter_cases import (assert_bit_equal, crafted, llr_k11_1, model_scored, mono_limit, run_both, scored_and_distinct, zipf_counts)
from universal_recommender_amd import _lib

N_BIG = 200_000   # users: cA cB << N for every candidate of the crafted rows (cA <= 6, cB <= 400)
SIZES = [100, 200, 300, 1500, 3000, 6000]   # distinct candidates per row: one-wave (two of them), 256 / 4Ki, 256 / 8Ki, 512 and 1024 threads


def P(k=50, min_llr=None, max_rows=100000):
    return O.DatasetParams(max_rows, k, min_llr)


def check(sess, mats, params, seed=3):
    """Oracle comparison (prefilter on), then on against off bit for bit.  Returns the per-event stats of the build with the prefilter."""
    _, _, stats = compare_with_oracle(sess, mats, params, seed)
    on, off = run_both(sess, mats, params, seed, run_device)
    assert_bit_equal(on, off)
    return stats


@pytest.fixture(scope="module")
def limits(sim_session):
    cache = {}

    def limit_of(ca, n_users=N_BIG):
        if (ca, n_users) not in cache:
            cache[(ca, n_users)] = mono_limit(sim_session, ca, n_users)
        return cache[(ca, n_users)]
    return limit_of


@pytest.fixture(scope="module")
def active_case():
    return crafted(np.random.default_rng(11), SIZES, ca=4, n_users=N_BIG)


def test_active_pruning_in_every_class(sim_session, active_case, limits):
    mats, rows = active_case
    stats = check(sim_session, mats, [P(), P()])
    bins = stats[1][0][1:8]
    assert bins[1] >= 2 and bins[2] >= 1 and bins[3] >= 1 and bins[4] >= 1 and bins[5] >= 1 and bins[0] == 0 and bins[6] == 0, bins
    scored, distinct = scored_and_distinct(sim_session, mats, [P(), P()], 3, run_device)
    want_scored, want_distinct = model_scored(rows, 50, limits)
    assert distinct[1] == want_distinct == sum(SIZES), (distinct, want_distinct)
    assert scored[1] == want_scored, (scored, want_scored)
    assert scored[1] < distinct[1] // 2, (scored, distinct)     # pruning ran, and removed most candidates
    assert scored[0] == distinct[0]                             # A'A here: rows of one pair (the micro class, which has no prefilter)


@pytest.mark.parametrize("k", [1, 7, 50, 64, 65])
def test_k(sim_session, limits, k):
    mats, rows = crafted(np.random.default_rng(100 + k), [130, 400, 1500], ca=3, n_users=N_BIG)
    check(sim_session, mats, [P(k), P(k)])
    scored, distinct = scored_and_distinct(sim_session, mats, [P(k), P(k)], 3, run_device)
    assert (scored[1], distinct[1]) == model_scored(rows, k, limits), (scored, distinct)
    assert scored[1] < distinct[1]


def test_ties_at_the_cut_are_decided_by_column(sim_session, limits):
    """>= 3 k candidates tied at cB == c*: all of them are kept and the existing select cuts them by column."""
    def cb_of(rng, n):
        cb = zipf_counts(rng, n)
        cb[cb <= 2] = 3
        cb[5:30] = 1         # 25 at cB = 1 (behind the k11 = 2 columns), then 160 at cB = 2: c* = 2
        cb[30:190] = 2
        return cb
    mats, rows = crafted(np.random.default_rng(21), [260, 900], ca=4, n_users=N_BIG, cb_of=cb_of)
    check(sim_session, mats, [P(), P()])
    scored, distinct = scored_and_distinct(sim_session, mats, [P(), P()], 3, run_device)
    assert (scored[1], distinct[1]) == model_scored(rows, 50, limits), (scored, distinct)
    assert scored[1] == 2 * (5 + 25 + 160), scored   # per row: the k11 = 2 columns and everything at or below the cut


def test_clamp_bin_and_no_k11_1(sim_session, limits):
    """Every candidate in the clamp bin (cB >= 255): no cut.  Every candidate with k11 >= 2: nothing to count."""
    mats, rows = crafted(np.random.default_rng(22), [150, 600], ca=4, n_users=N_BIG, cb_of=lambda rng, n: rng.integers(255, 400, n))
    check(sim_session, mats, [P(), P()])
    scored, distinct = scored_and_distinct(sim_session, mats, [P(), P()], 3, run_device)
    assert scored[1] == distinct[1] == 750 and model_scored(rows, 50, limits) == (750, 750)
    mats, rows = crafted(np.random.default_rng(23), [150, 600], ca=4, n_users=N_BIG, multi=10 ** 6)
    check(sim_session, mats, [P(), P()])
    scored, distinct = scored_and_distinct(sim_session, mats, [P(), P()], 3, run_device)
    assert scored[1] == distinct[1] == 750


def test_min_llr_cuts_inside_the_top_k(sim_session, active_case):
    mats, _ = active_case
    out = run_device(sim_session, mats, [P(), P()], 3)
    llr = out[1].to_host()[2]
    rp = out[1].to_host()[0]
    thr = float(np.median(llr[rp[0]:rp[1]]))      # the median score of the first row's top k: minLLR keeps about half of them
    stats = check(sim_session, mats, [P(50, thr), P(50, thr)])
    lens = np.diff(run_device(sim_session, mats, [P(50, thr), P(50, thr)], 3)[1].to_host()[0])
    assert 0 < lens[0] < 50, lens


def test_self_pair_and_unordered_rows(sim_session, sim_lib):
    """A'A with the self pair (rows whose self pair holds k11 = 1 included: cA = 1), Zipf data with N large; and URCCO_FLAG_UNORDERED_ROWS compared as sets."""
    rng = np.random.default_rng(31)
    a = rand_csr(rng, 60000, 3000, 6, zipf_s=1.1)
    b = rand_csr(rng, 60000, 9000, 14, zipf_s=1.0)
    stats = check(sim_session, [a, b], [P(20), P(20)])
    assert stats[0][0][2] > 0 and stats[1][0][2] > 0, (stats[0][0][1:8], stats[1][0][1:8])
    scored, distinct = scored_and_distinct(sim_session, [a, b], [P(20), P(20)], 3, run_device)
    assert scored[0] < distinct[0] and scored[1] < distinct[1], (scored, distinct)
    unordered_case(sim_lib, sim_session.device, [a, b], [P(20), P(20)])


def unordered_case(lib, device, mats, params, seed=3):
    """URCCO_FLAG_UNORDERED_ROWS (a context flag): rows are top-k SETS -- prefilter on against off and against the oracle, rows sorted."""
    from helpers import check_indicators, sort_rows, to_dev, to_params
    from universal_recommender_amd.device import Context, cross_occurrence_context
    ctx = Context(device, lib, flags=_lib.FLAG_UNORDERED_ROWS)
    try:
        def run(c, m, p, sd):
            out = cross_occurrence_context(c, [to_dev(x, device) for x in m], to_params(p), sd)
            return [type("Held", (), {"to_host": (lambda self, h=o.to_host(): h), "stats": o.stats.clone()})() for o in out]   # (a context reuses its output pool)
        on, off = run_both(ctx, mats, params, seed, run)
        assert_bit_equal(on, off, as_sets=True)
        for o, r in zip(on, O.cross_occurrence_downsampled(mats, params, seed)):
            check_indicators(sort_rows(o.to_host()), r)
    finally:
        ctx.close()


def test_small_n_the_table_forbids_pruning(sim_session):
    """N of 30-200 users, dense matrices: cA cB >= N for every pair, the limits are 0 or tiny, and no candidate may be dropped."""
    rng = np.random.default_rng(41)
    for n_users in (30, 120, 200):
        a_dense = rng.random((n_users, 40)) < 0.7
        b_dense = rng.random((n_users, 400)) < 0.5
        def csr(m):
            rp = np.zeros(m.shape[0] + 1, np.int64)
            np.cumsum(m.sum(1), out=rp[1:])
            return O.Csr(m.shape[0], m.shape[1], rp, np.nonzero(m)[1].astype(np.int32))
        mats = [csr(a_dense), csr(b_dense)]
        stats = check(sim_session, mats, [P(), P()])
        assert stats[1][0][1] == 0 and stats[1][0][7] == 0, stats[1][0][1:8]    # A'B: no micro row, no multi-pass row
        cb_min = int(b_dense.sum(0).min())
        lims = [mono_limit(sim_session, int(ca), n_users) for ca in np.unique(a_dense.sum(0))]
        assert max(lims) < cb_min, (lims, cb_min)          # the premise: the table forbids every drop
        scored, distinct = scored_and_distinct(sim_session, mats, [P(), P()], 3, run_device)
        assert scored == distinct, (n_users, scored, distinct)
    # Zipf data at small N (limits of a few units for small cA): results identical whatever is dropped
    for n_users in (60, 200):
        mats = [rand_csr(rng, n_users, 300, 8), rand_csr(rng, n_users, 3000, 40, zipf_s=0.6)]
        check(sim_session, mats, [P(), P(20)])


@pytest.mark.parametrize("n_users", [N_BIG, 600, 5000])
def test_limit_table_by_its_consequences(sim_session, n_users):
    """For sampled cA: the LLR of (k11 = 1, cA, cB) is strictly decreasing and positive up to the re-derived limit and not beyond -- and a row built
    around that limit (k + 1 candidates at cB = 1, then candidates on both sides of the limit) scores exactly the candidates the rule leaves."""
    for ca in (1, 2, 5, 17):
        m = mono_limit(sim_session, ca, n_users)
        assert m >= 2, (ca, n_users, m)
        f = llr_k11_1(sim_session, ca, np.arange(1, m + 2), n_users)
        assert np.all(f[:m - 1] > f[1:m]) and np.all(f[:m - 1] > 0.0)
        top = min(m + 1, 4096 - ca)
        if top == m + 1 and ca + m <= n_users:
            assert not (f[m - 1] > f[m] and f[m - 1] > 0.0), (ca, n_users, m)    # not beyond
        if m >= 254 or ca < 2:
            continue
        def cb_of(rng, n, m=m):
            cb = np.concatenate([np.ones(60, np.int64), np.arange(2, n - 60 + 2)])   # cB = 2 .. on both sides of m
            assert cb.max() > m + 3
            return cb
        mats, rows = crafted(np.random.default_rng(5), [m + 80], ca=ca, n_users=n_users, cb_of=cb_of, multi=0)
        check(sim_session, mats, [P(), P()])
        scored, distinct = scored_and_distinct(sim_session, mats, [P(), P()], 3, run_device)
        want = model_scored(rows, 50, lambda c: mono_limit(sim_session, c, n_users))
        assert (scored[1], distinct[1]) == want and scored[1] == 60 + (m + 80 - 60 - (m - 1)), (scored, distinct, want, m)
