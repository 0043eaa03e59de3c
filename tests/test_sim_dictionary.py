"""The device dictionary on the host simulator: the cases of tests/dictionary_cases.py -- constructed keys with chosen home slots, each result compared
exactly with a Python dict walked in stream order -- plus, without any device, the restated hash and capacity rule against the sources, and the whole
ingest path (this file, test_sim_ingest.py, test_sim_sorted_rows.py) once more under guard pages and with the waves of a block in reverse order.

The hot-key case runs as a smaller twin here (20 000 occurrences of the hot key, thresholds at 100: 80 000 positions, 120 000 with the masked ones; the
hardware driver's 200 000 / 1000 is 800 000 / 1 200 000 positions, 5 s of simulated threads and Python dict walks per run, and this file runs three times)."""
import os
import re
import subprocess
import sys

import pytest

import dictionary_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "universal-recommender_amd", "csrc")


def test_restated_hash_and_capacity_are_the_library_s():
    """ig_mix's two multipliers and three shift counts, IG_EMPTY, the capacity rule of urcco_dev_dictionary_build and SCAN_TILE, read out of the sources."""
    text = open(os.path.join(CSRC, "ingest_kernels.hip")).read()
    body = re.search(r"unsigned long long ig_mix\(unsigned long long x\) \{(.*?)\n\}", text, flags=re.S).group(1)
    assert tuple(int(s) for s in re.findall(r"x \^= x >> (\d+);", body)) == D.MIX_SHIFTS
    assert tuple(int(m, 16) for m in re.findall(r"x \*= 0x([0-9A-Fa-f]+)ull;", body)) == D.MIX_MULTIPLIERS
    steps = re.findall(r"x \^= x >> \d+;|x \*= 0x[0-9A-Fa-f]+ull;", body)
    assert [s[2] for s in steps] == ["^", "*", "^", "*", "^"], "shift, multiply, shift, multiply, shift"
    assert re.search(r"constexpr unsigned long long IG_EMPTY = ~0ull;", text) and D.RESERVED == 2 ** 64 - 1
    assert len(re.findall(r"ig_mix\(key\) & t\.mask", text)) == 2, "home slot = hash & mask, in ig_find and in the insert kernel"
    api = open(os.path.join(CSRC, "urcco_api.hip")).read()
    rule = re.search(r"int64_t cap = (\d+);\s*while \(cap < (\d+) \* n\) cap <<= 1;\s*tab->capacity = cap;\s*tab->t\.mask = \(unsigned long long\)cap - 1ull;", api)
    assert rule and (int(rule.group(1)), int(rule.group(2))) == (D.MIN_CAPACITY, 2)
    assert [D.capacity(n) for n in (0, 1, 512, 513, 1024, 1025)] == [1024, 1024, 1024, 2048, 2048, 4096]
    scan = open(os.path.join(CSRC, "cco_kernels.h")).read() + open(os.path.join(CSRC, "cco_misc.hip")).read()
    assert int(re.search(r"constexpr int(?:64_t)? SCAN_TILE = (\d+);", scan).group(1)) == D.SCAN_TILE
    # the inversion itself
    for x in (0, 1, 2 ** 63, 2 ** 64 - 2, 2 ** 64 - 1, 0x0123456789ABCDEF):
        assert D.unmix(D.mix(x)) == x and D.mix(D.unmix(x)) == x
    for cap, slot in ((1024, 1023), (1024, 0), (8192, 5)):
        assert all(D.home(k, cap) == slot for k in D.keys_at(slot, cap, 20))


def test_long_chain_that_wraps(sim_session):
    D.case_chain_that_wraps(sim_session)


@pytest.mark.parametrize("base", [0, D.SCAN_TILE - 32])
def test_one_wave_one_slot(sim_session, base):
    D.case_one_wave_one_slot(sim_session, base)


def test_hot_key_and_counts_on_the_threshold(sim_session):
    D.case_hot_key(sim_session, hot=20_000, threshold=100)


def test_sizes(sim_session):
    D.case_sizes(sim_session)


def test_first_positions_on_tile_edges(sim_session):
    D.case_tile_edges(sim_session)


def test_extreme_keys(sim_session):
    D.case_extreme_keys(sim_session)


@pytest.mark.parametrize("name", D.RESERVED_NAMES)
def test_reserved_key_is_refused(sim_session, name):
    D.case_reserved_key(sim_session, name)


def test_verify_counts_the_planted_collisions(sim_session):
    D.case_verify(sim_session)


def test_bad_arguments(sim_session):
    D.case_arguments(sim_session)


INGEST_FILES = [os.path.abspath(__file__), os.path.join(ROOT, "tests", "test_sim_ingest.py"), os.path.join(ROOT, "tests", "test_sim_sorted_rows.py")]


def _rerun(**env):
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", *INGEST_FILES], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True)
    assert r.returncode == 0, f"{env}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"


def test_under_guard_pages():
    """The whole ingest path once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument): a probe that
    walks off the table's last slot, a flag or prefix read past n, faults."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    _rerun(HIPSIM_GUARD="1")


def test_with_a_guard_page_before_every_buffer_and_waves_in_reverse():
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    _rerun(HIPSIM_GUARD="3", HIPSIM_ORDER="reverse")
