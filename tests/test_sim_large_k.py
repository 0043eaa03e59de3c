"""The whole k domain of the row kernels on the host simulator: the cases of tests/large_k_cases.py -- capacity edges of the five LDS classes at the largest k
that still cuts a row there (k = 169 .. 5460), rows between the edges with mixed k11 (k = 600 .. 5461), the dense global kernel at k = 1024 (radix select,
survivor arrays full) and from k = 1025 on (the argmax sweeps) -- each against the oracle, the class of every row asserted.

Shapes of the hardware driver (tests/test_gpu_large_k.py) that cost 8 to 21 s of CPU each here -- an argmax sweep is one pass of 1024 simulated threads,
about 1.6 ms -- run as smaller twins of the same construction (CPU time measured per case; the whole file: 33 s):
  * one above the E = 32768 edge at k = 5460 (5460 sweeps)       ->  the same edge at k = 1025: D = 10922 - 1025 + 1 = 9898 candidates, dense kernel (2.3 s per family);
  * (2 holders, 40 000 columns, 6 000 each) at k = 5460 and 5461,
    (2, 40 000, 12 000) at k = 10922 (8.4, 8.9 s; 10922 sweeps)  ->  2 holders of 500 out of 1200 columns at the same three k: the row keeps every candidate, class 5 /
                                                                     class 5 / dense kernel (0.1, 0.1, 1.6 s);
  * the 12 000-column dense problem at k = 20000                 ->  the same users on a B 400 columns wide at k = 1025 (tables), 10922 and 40000 (dense kernel): no row
                                                                     reaches k, every sweep loop ends at the `wk == 0` break (0.1, 0.8, 0.9 s).
"""
import pytest
import torch

import large_k_cases as C
from universal_recommender_amd import _lib


FAST_EDGES = [c for c in C.EDGES if c not in C.SLOW_ON_THE_SIMULATOR]


@pytest.mark.parametrize("E,family,which", FAST_EDGES, ids=[C.EDGE_ID(*c) for c in FAST_EDGES])
def test_capacity_edges(sim_session, E, family, which):
    C.case_edge(sim_session, E, family, which)


@pytest.mark.parametrize("family", ["hashed", "column"])
def test_one_above_the_last_table_at_a_smaller_k(sim_session, family):
    """The twin of (32768, family, "above"): D + k one above the edge of the largest table at k = 1025 -- bin 6, the dense global kernel's sweeps."""
    C.case_edge(sim_session, 32768, family, "above", k=1025)


@pytest.mark.parametrize("case", C.MIXED[:-3], ids=C.mixed_id)
def test_rows_between_the_edges(sim_session, case):
    C.case_mixed(sim_session, *case)


@pytest.mark.parametrize("case", C.MIXED_SMALL, ids=C.mixed_id)
def test_rows_with_fewer_candidates_than_a_huge_k(sim_session, case):
    """The twins of k = 5460, 5461 and 10922 of the hardware driver: two holders of 500 out of 1200 columns, so the row keeps every candidate."""
    C.case_mixed(sim_session, *case, cut=False)


@pytest.mark.parametrize("k", [1024, 1025])
def test_dense_global_kernel_around_gsel_k(sim_session, k):
    C.case_dense(sim_session, k)


def test_dense_global_kernel_with_min_llr(sim_session):
    C.case_dense(sim_session, 1025, min_llr=0.5)


@pytest.mark.parametrize("k", [1025, 10922, 40000])
def test_k_beyond_every_table_and_every_row(sim_session, k):
    """The twin of k = 10922 and k = 20000 of the hardware driver: B 400 columns wide, every row ends at the `wk == 0` break with emitted < k."""
    C.case_dense(sim_session, k, small=True)


def test_self_pair_in_the_dense_global_kernel(sim_session):
    C.case_self_pair(sim_session)


def test_argmax_sweeps_break_ties_by_column(sim_session):
    C.case_sweep_ties(sim_session)


@pytest.mark.parametrize("flags", [0, _lib.FLAG_UNORDERED_ROWS], ids=["ordered", "unordered"])
@pytest.mark.parametrize("k", [600, 1024, 1025])
def test_context_level(sim_lib, k, flags):
    C.case_context(sim_lib, torch.device("cpu"), k, flags)
