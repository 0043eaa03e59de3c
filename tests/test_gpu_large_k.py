"""The whole k domain of the row kernels on hardware: the full list of tests/large_k_cases.py -- capacity edges of the five LDS classes at the largest k that
still cuts a row there (k = 169 .. 5460; one above the last edge: the dense global kernel), rows between the edges with mixed k11 (k = 600 .. 10922), the dense
global kernel at k = 1024 (radix select, survivor arrays full), from k = 1025 on (the argmax sweeps) and at a k no row reaches -- each against the oracle,
the class of every row asserted, and each run twice: the two outputs must be byte-identical."""
import pytest

import large_k_cases as C
from universal_recommender_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("E,family,which", C.EDGES, ids=[C.EDGE_ID(*c) for c in C.EDGES])
def test_capacity_edges(gpu_session, E, family, which):
    C.case_edge(gpu_session, E, family, which, repeat=True)


@pytest.mark.parametrize("family", ["hashed", "column"])
def test_one_above_the_last_table_at_a_smaller_k(gpu_session, family):
    C.case_edge(gpu_session, 32768, family, "above", k=1025, repeat=True)


@pytest.mark.parametrize("case", C.MIXED, ids=C.mixed_id)
def test_rows_between_the_edges(gpu_session, case):
    C.case_mixed(gpu_session, *case, repeat=True)


@pytest.mark.parametrize("case", C.MIXED_SMALL, ids=C.mixed_id)
def test_rows_with_fewer_candidates_than_a_huge_k(gpu_session, case):
    C.case_mixed(gpu_session, *case, repeat=True, cut=False)


@pytest.mark.parametrize("k", [1024, 1025, 20000])
def test_dense_global_kernel_around_and_far_beyond_gsel_k(gpu_session, k):
    C.case_dense(gpu_session, k, repeat=True)


def test_dense_global_kernel_with_min_llr(gpu_session):
    C.case_dense(gpu_session, 1025, min_llr=0.5, repeat=True)


@pytest.mark.parametrize("k", [1025, 10922, 40000])
def test_k_beyond_every_table_and_every_row(gpu_session, k):
    C.case_dense(gpu_session, k, small=True, repeat=True)


def test_self_pair_in_the_dense_global_kernel(gpu_session):
    C.case_self_pair(gpu_session, repeat=True)


def test_argmax_sweeps_break_ties_by_column(gpu_session):
    C.case_sweep_ties(gpu_session, repeat=True)


@pytest.mark.parametrize("flags", [0, _lib.FLAG_UNORDERED_ROWS], ids=["ordered", "unordered"])
@pytest.mark.parametrize("k", [600, 1024, 1025])
def test_context_level(gpu_session, k, flags):
    C.case_context(gpu_session.lib, gpu_session.device, k, flags, repeat=True)
