"""The direct ranking of the packed row kernels (csrc/cco_rows.hip: rows with k < C <= direct_limit valid candidates skip the select) on hardware: the cases
of tests/direct_rank_cases.py -- each compared with the oracle and, bit for bit, with the same build under NO_DIRECT_RANK; COUNT_DIRECT against the model --
and one realistic mix."""
import numpy as np
import pytest

import direct_rank_cases as C
from oracle import c_oracle as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("multi", [0, 5])
@pytest.mark.parametrize("c", [1, 2, 3, 4, 5])
def test_edges_of_the_condition(gpu_session, c, multi):
    C.case_edges(gpu_session, c, multi)


def test_without_the_prefilter_in_front(gpu_session):
    C.case_no_prefilter(gpu_session)


def test_ties_are_cut_by_column(gpu_session):
    C.case_ties(gpu_session)


@pytest.mark.parametrize("k", [7, 64, 65])
def test_small_and_odd_k(gpu_session, k):
    C.case_k(gpu_session, k)


def test_min_llr_moves_a_row_inside_the_limit(gpu_session):
    C.case_min_llr(gpu_session)


def test_self_pair_and_unordered_rows(gpu_session):
    C.case_self_pair_and_unordered(gpu_session, gpu_session.lib)


def test_realistic_mix(gpu_session):
    """synth.config3(0.1), two event types: every row against the oracle, on against off bit for bit, and rows ranked directly in both event types (the test
    cannot pass with the path dead; the one-wave class, whose direct ranking is compiled out -- direct_limit --, adds none of them)."""
    from universal_recommender_amd import synth
    cfg = synth.config3(0.1)
    data = synth.generate(cfg)[:2]
    mats = [O.Csr(cfg.n_users, nc, rp, ci.astype(np.int32)) for (_, nc, rp, ci) in data]
    params = [O.DatasetParams(500, 50, None) for _ in mats]
    bins = C.check(gpu_session, mats, params, seed=1)
    got = C.direct_rows(gpu_session, mats, params, 1)
    print(f"rows by class {[b.tolist() for b in bins]}; rows ranked directly per event type {got}")
    assert bins[0][1] > 0 and bins[1][1] > 0, bins
    assert got[0] > 0 and got[1] > 0, got
