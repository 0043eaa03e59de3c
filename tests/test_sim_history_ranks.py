"""urcco_dev_history_ranks / urcco_dev_fill_order on the host simulator (kernel LOGIC on the CPU) against the contract of include/urcco.h restated in numpy
(tests/history_ranks_cases.py): the popular / trending / hot ranks of the items from event streams, and the backfill order from up to four rank fields.
Every output has exactly its size, so the rerun under HIPSIM_GUARD faults on a write past either end, and on a read past a stream, a column map, a rank
field or the scratch (count tables, key and id buffers, histograms)."""
import os
import subprocess
import sys

import history_ranks_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_interval_bounds(sim_session):
    R.boundary_cases(sim_session)


def test_open_window_and_no_end(sim_session):
    R.open_window_cases(sim_session)


def test_ids_and_column_maps(sim_session):
    R.id_cases(sim_session)


def test_streams(sim_session):
    R.stream_cases(sim_session)


def test_block_cache_paths(sim_session):
    R.cache_cases(sim_session)


def test_rank_bad_arguments(sim_session):
    R.rank_bad_argument_cases(sim_session)


def test_fill_order_sizes(sim_session):
    R.fill_size_cases(sim_session)


def test_fill_order_digit_skip(sim_session):
    R.fill_digit_cases(sim_session)


def test_fill_order_stability_and_fields(sim_session):
    R.fill_stability_cases(sim_session)


def test_fill_order_bad_arguments(sim_session):
    R.fill_bad_argument_cases(sim_session)


def test_one_field_is_the_order_of_from_indicators(sim_session):
    R.from_indicators_case(sim_session)


def test_under_guard_pages():
    """This module once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument)."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    env = dict(os.environ, HIPSIM_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
