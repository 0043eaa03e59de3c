"""urcco_dev_props_compact on the host simulator (kernel LOGIC on the CPU) against the contract of include/urcco.h restated in numpy
(tests/props_compact_cases.py): one property's stream without the values no item's state names any more, and a store that answers as before.  Every
input and output has exactly its size (K, K + 1, V), so the rerun under HIPSIM_GUARD faults on an access past either end of a stream, a state array,
the value arrays, an output or the scratch."""
import os
import subprocess
import sys

import props_compact_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slice_class_edges(sim_session):
    CC.slice_cases(sim_session)


def test_copy_tiles(sim_session):
    CC.tile_cases(sim_session)


def test_one_item_owns_the_stream(sim_session):
    CC.owner_case(sim_session)


def test_every_winner_dead(sim_session):
    CC.dead_case(sim_session)


def test_item_and_event_domain(sim_session):
    CC.domain_cases(sim_session)


def test_malformed_state_stays_inside_the_arrays(sim_session):
    CC.malformed_cases(sim_session)


def test_bad_arguments(sim_session):
    CC.bad_argument_cases(sim_session)


def test_compacted_store_and_its_twin(sim_session):
    CC.twin_case(sim_session)


def test_compacted_properties_through_batch_predict(sim_session):
    CC.predict_case(sim_session)


def test_under_guard_pages():
    """This module once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument)."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    env = dict(os.environ, HIPSIM_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
