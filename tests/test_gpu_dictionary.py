"""The device dictionary on hardware: the cases of tests/dictionary_cases.py at their full shapes, each run twice with identical results; the two
cases that live on contention -- 64 keys of one wave on one empty slot, a key with 200 000 occurrences -- build the same stream ten times and want ten
identical tables of ids (the CAS and the stale-read shortcuts of ig_insert_kernel only exist here)."""
import pytest

import dictionary_cases as D

pytestmark = pytest.mark.gpu


def test_long_chain_that_wraps(gpu_session):
    D.case_chain_that_wraps(gpu_session, repeat=2)


@pytest.mark.parametrize("base", [0, D.SCAN_TILE - 32])
def test_one_wave_one_slot(gpu_session, base):
    D.case_one_wave_one_slot(gpu_session, base, repeat=10)


def test_hot_key_and_counts_on_the_threshold(gpu_session):
    D.case_hot_key(gpu_session, repeat=10)


def test_sizes(gpu_session):
    D.case_sizes(gpu_session, repeat=2)


def test_first_positions_on_tile_edges(gpu_session):
    D.case_tile_edges(gpu_session, repeat=2)


def test_extreme_keys(gpu_session):
    D.case_extreme_keys(gpu_session, repeat=2)


@pytest.mark.parametrize("name", D.RESERVED_NAMES)
def test_reserved_key_is_refused(gpu_session, name):
    D.case_reserved_key(gpu_session, name, repeat=2)


def test_verify_counts_the_planted_collisions(gpu_session):
    D.case_verify(gpu_session, repeat=2)


def test_bad_arguments(gpu_session):
    D.case_arguments(gpu_session)
