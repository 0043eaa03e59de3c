"""The host level's boundary check on the host simulator: the cases of tests/boundary_check_cases.py at the simulator's CU count (8 CUs: 128 blocks, so
the second grid round starts at row 16 384 / 4 096 / 512 for G = 2 / 8 / 64).  In-range violations as on hardware; out-of-range columns and corrupt
row_ptr entries only here (a hole in the check would send the build behind it out of bounds), and those, with the false-positive control, once more
under guard pages behind and before every buffer.

A shard with rp0 != 0: the process-wide entry point drives several GPUs only through RCCL communicators (urcco_context_create without caller-supplied
collectives), which the simulator does not have.  The same staging code (urcco_context_stage) is reached with 2 and 3 simulated devices through
urcco_context_cross_occurrence on a caller-made context whose collectives are looped back in-process: the in-range cases in the first and the last row
of the second shard run there."""
import os
import re
import subprocess
import sys

import pytest

import boundary_check_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS = (2, 8, 64)


def sim_cus():
    text = open(os.path.join(ROOT, "tests", "hostsim", "include", "hip", "hip_runtime.h")).read()
    return int(re.search(r"multiProcessorCount = (\d+);", text).group(1))


N_CU = sim_cus()


@pytest.fixture(scope="module")
def host_lib(sim_lib):
    try:
        yield sim_lib
    finally:
        sim_lib.urcco_shutdown()


IN_RANGE = [(G, kind, place, t) for G in GS for kind in B.KINDS for place in B.PLACES for t in B.offsets(G)]


@pytest.mark.parametrize("G,kind,place,t", IN_RANGE, ids=["G{}-{}-{}-t{}".format(*c) for c in IN_RANGE])
def test_in_range_violation_is_counted_once(host_lib, G, kind, place, t):
    B.case_in_range(host_lib, N_CU, G, kind, place, t)


@pytest.mark.parametrize("G", GS)
def test_all_planted_at_once(host_lib, G):
    assert B.case_all_at_once(host_lib, N_CU, G) >= 16


@pytest.mark.parametrize("bad_dataset", [1, 2])
def test_violation_in_a_secondary(host_lib, bad_dataset):
    B.case_secondary(host_lib, N_CU, bad_dataset)


@pytest.mark.parametrize("G", [2, 8])
def test_control_first_column_below_the_previous_row_s_last(host_lib, G):
    B.case_first_column_below_previous_last(host_lib, G)


@pytest.mark.parametrize("place", B.PLACES)
@pytest.mark.parametrize("what", list(B.OUT_OF_RANGE))
@pytest.mark.parametrize("G", GS)
def test_out_of_range_column(host_lib, G, what, place):
    B.case_out_of_range(host_lib, N_CU, G, what, place)


@pytest.mark.parametrize("what", ["lowered", "above nnz", "decrease that cancels out"])
@pytest.mark.parametrize("G", GS)
def test_row_ptr(host_lib, G, what):
    B.case_row_ptr(host_lib, N_CU, G, what)


@pytest.fixture(scope="module")
def shard_context(sim_lib):
    """get(n): a context over n simulated devices, collectives looped back in-process; made once per n, closed with the module."""
    import torch
    from universal_recommender_amd import sharded
    from universal_recommender_amd.device import Context
    before, made = os.environ.get("HIPSIM_DEVICE_COUNT"), {}

    def get(n):
        if n not in made:
            os.environ["HIPSIM_DEVICE_COUNT"] = str(max([n] + list(made)))
            coll = sharded.TorchCollectives(n, list(range(n)))
            made[n] = (Context(torch.device("cpu"), sim_lib, n_gpus=n, collectives=coll), coll)
        return made[n][0]
    try:
        yield get
        assert all(coll.error is None for _, coll in made.values())
    finally:
        for ctx, _ in made.values():
            ctx.close()
        if before is None:
            os.environ.pop("HIPSIM_DEVICE_COUNT", None)
        else:
            os.environ["HIPSIM_DEVICE_COUNT"] = before


# three devices (the second shard is an inner one) at G = 8 only: a simulated build costs 70 ms whatever its size
@pytest.mark.parametrize("place", ["first row of the second shard", "last row of the second shard"])
@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("n,G", [(2, 2), (2, 8), (2, 64), (3, 8)])
def test_violation_in_a_shard_with_a_row_ptr_base(sim_lib, shard_context, n, G, kind, place):
    B.case_shard(sim_lib, shard_context(n), n, G, kind, place)


@pytest.mark.parametrize("mode", ["1", "3"])
def test_under_guard_pages(mode):
    """The out-of-range, row_ptr and control cases once more with every buffer ending at (1) / starting behind (3) a PROT_NONE page (tests/test_sim_guard.py
    describes the instrument): a walk that follows a corrupt row_ptr, or a read of col_idx[-1], faults."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "out_of_range or row_ptr or control or at_once"], cwd=ROOT, env=dict(os.environ, HIPSIM_GUARD=mode), capture_output=True, text=True)
    assert r.returncode == 0, f"HIPSIM_GUARD={mode}: rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
