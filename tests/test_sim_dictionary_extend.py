"""The growable device dictionary on the host simulator: the cases of tests/dictionary_extend_cases.py -- constructed keys with chosen home slots, every
result compared exactly with a Python dict walked in stream order and with one dictionary_build over all batches laid end to end -- and the whole file once
more under guard pages: `ids` and `new_pos` are then buffers of exactly n entries that end at a PROT_NONE page, as are the scratch arrays in the arena."""
import os
import subprocess
import sys

import pytest

import dictionary_extend_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_batches", [1, 2, 7])
def test_one_stream_in_batches(sim_session, n_batches):
    X.case_batching(sim_session, n_batches)


def test_growth_on_the_capacity_rule(sim_session):
    X.case_growth(sim_session)


def test_chain_that_wraps_is_rehashed(sim_session):
    X.case_chain_wraps_then_rehash(sim_session)


def test_new_keys_in_old_chains(sim_session):
    X.case_new_keys_in_old_chains(sim_session)


@pytest.mark.parametrize("base", [0, X.D.SCAN_TILE - 32])
def test_one_wave_one_slot(sim_session, base):
    X.case_one_wave_one_slot(sim_session, base)


def test_one_key_a_hundred_thousand_times(sim_session):
    X.case_hot_key(sim_session)


def test_first_appearances_on_tile_edges(sim_session):
    X.case_tile_edges(sim_session)


def test_select(sim_session):
    X.case_select(sim_session)


def test_extreme_keys(sim_session):
    X.case_extreme_keys(sim_session)


@pytest.mark.parametrize("grows", [False, True])
def test_refusals_leave_the_table_as_it_was(sim_session, grows):
    X.case_refusals(sim_session, grows)


def test_table_of_min_count_2_is_refused(sim_session):
    X.case_min_count_table_is_refused(sim_session)


def test_collisions_are_counted_and_raised(sim_session):
    X.case_collisions(sim_session)


def test_ids_may_be_null_and_batches_empty(sim_session):
    X.case_nullable_ids_and_empty_batches(sim_session)


def test_under_guard_pages():
    """This file once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument): a probe that walks off the
    table's last slot, a rank beyond the firsts, a flag or prefix read past n, faults."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)], cwd=ROOT,
                       env=dict(os.environ, HIPSIM_GUARD="1"), capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
