"""urcco_dev_history_users / urcco_dev_history_matrix on the host simulator (kernel LOGIC on the CPU) against the contract of include/urcco.h restated in
numpy (tests/history_matrix_cases.py): which users train, and the user x column matrix of an event type from its stream and its index alone.  out_row_ptr
has exactly n_rows + 1 and out_col_idx exactly `capacity` entries, so the rerun under HIPSIM_GUARD faults on a write past either, and on a read past the
index entries, the stream or the scratch (raw rows, lists, bitmaps)."""
import os
import subprocess
import sys

import history_matrix_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_class_edges(sim_session):
    M.edge_cases(sim_session)


def test_window(sim_session):
    M.window_cases(sim_session)


def test_users(sim_session):
    M.user_cases(sim_session)


def test_several_heavy_rows_per_block(sim_session):
    M.heavy_rows_case(sim_session)


def test_capacity(sim_session):
    M.capacity_cases(sim_session)


def test_hostile_index(sim_session):
    M.hostile_cases(sim_session)


def test_against_csr_from_pairs(sim_session):
    M.pairs_cases(sim_session)


def test_bad_arguments(sim_session):
    M.bad_argument_cases(sim_session)


def test_under_guard_pages():
    """This module once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument)."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    env = dict(os.environ, HIPSIM_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
