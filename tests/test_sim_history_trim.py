"""urcco_dev_history_trim on the host simulator (kernel LOGIC on the CPU) against the contract of include/urcco.h restated in numpy
(tests/history_trim_cases.py): the stream and the index without the events older than a cut-off and without the events of listed users.  Every output
buffer has exactly the size the restatement gives (K, KE, n_users + 1), so the rerun under HIPSIM_GUARD faults on a write past out_items[K],
out_times[K], out_pos[KE] or out_row_ptr[n_users + 1], and on a read past the index entries or the scratch bitmaps."""
import os
import subprocess
import sys

import history_trim_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_word_edges(sim_session):
    T.word_cases(sim_session)


def test_time_rule(sim_session):
    T.time_cases(sim_session)


def test_users(sim_session):
    T.user_cases(sim_session)


def test_user_of_more_than_one_round_of_chunks(sim_session):
    """One listed user of more entries than the mark kernel's blocks take in one round of chunks"""
    T.user_cases(sim_session, big=T.BIG_USER)


def test_hostile_index(sim_session):
    T.hostile_cases(sim_session)


def test_rows_over_a_trimmed_history(sim_session):
    T.rows_case(sim_session)


def test_trim_append_trim(sim_session):
    T.chain_case(sim_session)


def test_bad_arguments(sim_session):
    T.bad_argument_cases(sim_session)


def test_under_guard_pages():
    """This module once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument)."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    env = dict(os.environ, HIPSIM_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
