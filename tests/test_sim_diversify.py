"""urcco_dev_diversify on the host simulator (kernel LOGIC on the CPU) against the greedy MMR rule of decision D36 (tests/diversify_cases.py): its cases,
the constructed matrices, the arguments, and the stream audit.  tests/test_gpu_diversify.py runs the same tests, bar the audit, on the MI355X."""
import ctypes as C

import pytest

import diversify_cases as D


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: "-".join(map(str, c)))
def test_rule(sim_session, case):
    D.check_case(sim_session, case)


def test_constructed(sim_session):
    D.check_constructed(sim_session)


def test_arguments(sim_session):
    D.check_arguments(sim_session)


def test_no_null_stream_operation(sim_session, sim_lib):
    sim_lib.hipsim_null_stream_ops.restype = C.c_longlong
    before = int(sim_lib.hipsim_null_stream_ops())
    D.run(sim_session, D.problem(21, 6, 70, 20, 0.25))
    assert int(sim_lib.hipsim_null_stream_ops()) == before
