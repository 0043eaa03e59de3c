"""urcco_dev_props_* on the host simulator (kernel LOGIC on the CPU) against the rule of include/urcco.h restated in plain Python (tests/props_ref.py;
the cases are tests/props_cases.py): $set / $unset / $delete events aggregated into the state words, and the rows, dates and mask cut from them.
Every input and output has exactly its size, so the rerun under HIPSIM_GUARD faults on an access past either end of a stream, a state array, the value
arrays, an output or the scratch."""
import os
import subprocess
import sys

import props_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ties_and_revival(sim_session):
    PC.tie_cases(sim_session)


def test_batching_and_permutations(sim_session):
    PC.batching_cases(sim_session)


def test_time_and_item_domain(sim_session):
    PC.domain_cases(sim_session)


def test_rows_class_edges_and_capacity(sim_session):
    PC.rows_cases(sim_session)


def test_malformed_state_stays_inside_the_arrays(sim_session):
    PC.malformed_state_cases(sim_session)


def test_contention_on_one_item(sim_session):
    PC.contention_case(sim_session)


def test_bad_arguments(sim_session):
    PC.bad_argument_cases(sim_session)


def test_numpy_form_of_the_reference():
    PC.numpy_reference_case()


def test_under_guard_pages():
    """This module once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument)."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    env = dict(os.environ, HIPSIM_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
