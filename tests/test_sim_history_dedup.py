"""urcco_dev_history_dedup on the host simulator (kernel LOGIC on the CPU) against the contract of include/urcco.h restated in numpy
(tests/history_dedup_cases.py).  Every output buffer has exactly the size the restatement gives (K, KE, n_users + 1), so the rerun under HIPSIM_GUARD
faults on a write past the results and on a read past the index entries or the scratch."""
import os
import subprocess
import sys

import pytest

import history_dedup_cases as D


@pytest.mark.parametrize("keep", sorted(D.KEEPS))
@pytest.mark.parametrize("case", D.CASES, ids=D.IDS)
def test_dedup(sim_session, case, keep):
    case[0](sim_session, keep, *case[1])


def test_under_guard_pages():
    """This module once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument)."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=dict(os.environ, HIPSIM_GUARD="1"), capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
