"""The direct ranking of the packed row kernels (csrc/cco_rows.hip: rows with k < C <= direct_limit valid candidates skip the select) on the host simulator.
Every case (tests/direct_rank_cases.py) compares the build with the oracle AND, bit for bit (row lengths, ids in order, LLR bits), with the same build under
NO_DIRECT_RANK; COUNT_DIRECT must report exactly the rows a plain-numpy model of the condition names.  The last test runs the cases once more on the
bounds-checked build with the waves of a block scheduled in reverse.  (The realistic mix of the issue, synth.config3(0.1), runs on hardware only:
tests/test_gpu_direct_rank.py -- tens of millions of pairs are minutes of simulator time.)"""
import os
import subprocess
import sys

import pytest

import direct_rank_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("multi", [0, 5])
@pytest.mark.parametrize("c", [1, 2, 3, 4, 5])
def test_edges_of_the_condition(sim_session, c, multi):
    C.case_edges(sim_session, c, multi)


def test_without_the_prefilter_in_front(sim_session):
    C.case_no_prefilter(sim_session)


def test_ties_are_cut_by_column(sim_session):
    C.case_ties(sim_session)


@pytest.mark.parametrize("k", [7, 64, 65])
def test_small_and_odd_k(sim_session, k):
    C.case_k(sim_session, k)


def test_min_llr_moves_a_row_inside_the_limit(sim_session):
    C.case_min_llr(sim_session)


def test_self_pair_and_unordered_rows(sim_session, sim_lib):
    C.case_self_pair_and_unordered(sim_session, sim_lib)


def test_bounds_checked_build_with_reversed_waves(sim_lib):
    """-fsanitize=bounds on every `__shared__` array index, guard pages behind every buffer, and the highest wave of a block first between two rendezvous:
    the set of a directly ranked row overlays the expand operands and the prefilter's histogram in two classes."""
    if os.environ.get("HIPSIM_VARIANT") == "bounds":
        pytest.skip("this IS the bounds-checked run")
    env = dict(os.environ, HIPSIM_VARIANT="bounds", HIPSIM_GUARD="1", HIPSIM_ORDER="reverse")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.join("tests", "test_sim_direct_rank.py"), "-k",
                        "edges or ties or min_llr or without"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
