"""The small-row body with eight pairs and two users per lane (csrc/cco_rows.hip, cco_rows_small_kernel<8, 2>: the one-wave class's rows of <= 128 users,
the small-block class's rows of <= 128 users and <= 512 pairs) on the host simulator.  Every case (tests/block_small_wave_cases.py) compares the build with
the oracle AND, bit for bit (row lengths, ids in order, LLR bits), with the same build under NO_BLOCK_SMALL_WAVE; COUNT_BLOCK_SMALL_WAVE must report exactly
the rows -- of the body and of its fallback, per list -- that a plain-numpy model of the sub-list rule names.  The last test runs cases once more on the
bounds-checked build with the waves of a block scheduled in reverse.  (The realistic mix of synth.config3(0.1) and the production default run on hardware
only: tests/test_gpu_block_small_wave.py.)"""
import os
import subprocess
import sys

import pytest

import block_small_wave_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_user_count_boundaries_with_empty_rows(sim_session):
    C.case_user_boundaries(sim_session)


def test_pair_count_boundaries(sim_session):
    C.case_pair_boundaries(sim_session)


def test_survivor_counts_around_64(sim_session):
    C.case_survivor_counts(sim_session)


def test_fallback_shapes(sim_session):
    C.case_fallback_shapes(sim_session)


@pytest.mark.parametrize("k", [1, 7, 50, 63, 64, 65])
def test_k_domain(sim_session, k):
    C.case_k(sim_session, k)


def test_min_llr_removes_part_of_a_row(sim_session):
    C.case_min_llr(sim_session)


def test_self_pair_mixed_sizes_and_unordered_rows(sim_session, sim_lib):
    C.case_self_pair_and_unordered(sim_session, sim_lib)


def test_column_addressed_accumulator(sim_session):
    C.case_column_addressed(sim_session)


def test_packed_and_plain_forms_agree(sim_session):
    C.case_plain_form(sim_session)


def test_older_counting_bits_on_a_mixed_build(sim_session):
    C.case_counting_bits(sim_session)


def test_bounds_checked_build_with_reversed_waves(sim_lib):
    """-fsanitize=bounds on every `__shared__` array index, guard pages behind every buffer, and the highest wave of a block first between two rendezvous: the
    body's marks, histogram, staged survivors and fallback keys share one region of LDS by phase, and the fallback parks columns in the accumulator."""
    if os.environ.get("HIPSIM_VARIANT") == "bounds":
        pytest.skip("this IS the bounds-checked run")
    env = dict(os.environ, HIPSIM_VARIANT="bounds", HIPSIM_GUARD="1", HIPSIM_ORDER="reverse")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.join("tests", "test_sim_block_small_wave.py"), "-k",
                        "user_count or pair_count or survivor or fallback_shapes"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
