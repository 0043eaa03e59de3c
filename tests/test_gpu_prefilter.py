"""The k11 = 1 prefilter of the packed row kernels (csrc/cco_rows.hip) on hardware: the smallest shapes that reach every accumulator class, each compared
with the oracle and, bit for bit (row lengths, ids in order, LLR bits), with the same build run with the prefilter switched off."""
import numpy as np
import pytest

from helpers import compare_with_oracle, rand_csr, run_device
from oracle import c_oracle as O
from prefilter_cases import assert_bit_equal, crafted, mono_limit, run_both, scored_and_distinct

pytestmark = pytest.mark.gpu


def P(k=50, max_rows=500):
    return O.DatasetParams(max_rows, k, None)


def check(sess, mats, params, seed):
    _, _, stats = compare_with_oracle(sess, mats, params, seed)
    on, off = run_both(sess, mats, params, seed, run_device)
    assert_bit_equal(on, off)
    return [s[0][1:8] for s in stats]      # rows by accumulator class, per event type


def test_zipf_catalogue_micro_to_256_threads(gpu_session):
    """200K users x 20K / 30K items, Zipf: the micro, one-wave and both 256-thread classes; pruning removes most of the candidates."""
    rng = np.random.default_rng(20261)
    mats = [rand_csr(rng, 200_000, 20_000, 6), rand_csr(rng, 200_000, 30_000, 8)]
    bins = check(gpu_session, mats, [P(), P()], 17)
    for b in bins:
        assert b[0] > 0 and b[1] > 0 and b[2] > 0 and b[3] > 0, bins
    scored, distinct = scored_and_distinct(gpu_session, mats, [P(), P()], 17, run_device)
    assert scored[0] < distinct[0] and scored[1] < distinct[1], (scored, distinct)


def test_dense_primary_512_and_1024_threads(gpu_session):
    """50K users x 2K items with a dense primary and a wider secondary: the rows of A'B hold more than 8192 pairs and land in the 512-thread class
    (up to 5.4K distinct columns) and the 1024-thread class (more); A'A stays in the 256-thread / 8Ki class."""
    rng = np.random.default_rng(20262)
    mats = [rand_csr(rng, 50_000, 2_000, 25, zipf_s=0.8), rand_csr(rng, 50_000, 8_000, 30, zipf_s=0.9)]
    bins = check(gpu_session, mats, [P(), P()], 18)
    assert bins[0][3] > 0 and bins[1][4] > 0 and bins[1][5] > 0, bins
    scored, distinct = scored_and_distinct(gpu_session, mats, [P(), P()], 18, run_device)
    assert scored[1] <= distinct[1] and scored[0] <= distinct[0], (scored, distinct)


def test_crafted_rows_of_every_class(gpu_session):
    """Rows of 100 .. 6000 distinct candidates, almost all k11 = 1, N large: every class from one wave to 1024 threads prunes."""
    mats, rows = crafted(np.random.default_rng(11), [100, 200, 300, 1500, 3000, 6000], ca=4, n_users=200_000)
    bins = check(gpu_session, mats, [P(50, 100000), P(50, 100000)], 3)
    assert bins[1][1] >= 2 and min(bins[1][2:6]) >= 1, bins
    scored, distinct = scored_and_distinct(gpu_session, mats, [P(50, 100000), P(50, 100000)], 3, run_device)
    assert distinct[1] == 11100 and scored[1] < distinct[1] // 2, (scored, distinct)


def test_small_n_the_table_forbids_pruning(gpu_session):
    """150 users, dense matrices: cA cB >= N for every pair; the limits are tiny and nothing may be dropped."""
    rng = np.random.default_rng(41)
    n_users = 150
    a_dense = rng.random((n_users, 40)) < 0.7
    b_dense = rng.random((n_users, 400)) < 0.5

    def csr(m):
        rp = np.zeros(m.shape[0] + 1, np.int64)
        np.cumsum(m.sum(1), out=rp[1:])
        return O.Csr(m.shape[0], m.shape[1], rp, np.nonzero(m)[1].astype(np.int32))
    mats = [csr(a_dense), csr(b_dense)]
    bins = check(gpu_session, mats, [P(50, 100000), P(50, 100000)], 3)
    assert bins[1][0] == 0 and bins[1][6] == 0, bins
    lims = [mono_limit(gpu_session, int(ca), n_users) for ca in np.unique(a_dense.sum(0))]
    assert max(lims) < int(b_dense.sum(0).min()), lims
    scored, distinct = scored_and_distinct(gpu_session, mats, [P(50, 100000), P(50, 100000)], 3, run_device)
    assert scored == distinct, (scored, distinct)
