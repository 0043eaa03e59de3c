"""urcco_dev_history_cap on the host simulator (kernel LOGIC on the CPU) against the contract of include/urcco.h restated in numpy
(tests/history_cap_cases.py): the trim with a per-user bound on the stored events.  Every output buffer has exactly the size the restatement gives
(K, KE, n_users + 1), so the rerun under HIPSIM_GUARD faults on a write past the results and on a read past the index entries or the scratch."""
import os
import subprocess
import sys

import history_cap_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segment_lengths_and_caps(sim_session):
    C.segment_cases(sim_session)


def test_times(sim_session):
    C.time_cases(sim_session)


def test_one_user_owns_the_stream(sim_session):
    C.big_owner_case(sim_session)


def test_index_order(sim_session):
    C.index_order_case(sim_session)


def test_no_cap_is_the_trim(sim_session):
    C.no_cap_cases(sim_session)


def test_rules_are_independent(sim_session):
    C.independence_case(sim_session)


def test_degenerate_input(sim_session):
    C.degenerate_cases(sim_session)


def test_hostile_index(sim_session):
    C.hostile_cases(sim_session)


def test_bad_arguments(sim_session):
    C.bad_argument_cases(sim_session)


def test_rows_below_the_cap_are_unchanged(sim_session):
    C.rows_unchanged_case(sim_session)


def test_capped_history_through_batch_predict(sim_session):
    C.predict_case(sim_session)


def test_schedule_on_one_history(sim_session):
    C.schedule_case(sim_session)


def test_under_guard_pages():
    """This module once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument)."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    env = dict(os.environ, HIPSIM_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
