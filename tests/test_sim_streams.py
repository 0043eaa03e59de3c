"""The stream audit of the host simulator (tests/hostsim: hipsim_null_stream_ops): a session of the simulator holds a stream the library created, never the
null stream, so every launch, copy, memset, event record or wait that a session-level call issues with the null stream -- or with no stream argument at all,
which HIP defaults to the null stream -- is an operation off the session's stream.  Next to hipStreamNonBlocking streams such an operation is ordered with
nothing.  One existing case per family of the session level (tests/stream_cases.py FAMILIES) runs unchanged; the counter must not move, and the first offender
is named when it does.  tests/test_gpu_streams.py runs the same cases on a caller's non-blocking stream on the MI355X."""
import ctypes as C

import pytest
import torch

import stream_cases as S


@pytest.fixture()
def audit(sim_lib):
    import os
    assert os.environ.get("URCCO_DEBUG_POISON", "0") in ("", "0"), "under URCCO_DEBUG_POISON the simulator does not count the blocking hipMemset: the audit would have a hole"
    sim_lib.hipsim_null_stream_ops.restype = C.c_longlong
    sim_lib.hipsim_null_stream_first.restype = C.c_char_p
    sim_lib.hipsim_null_stream_reset.restype = None
    sim_lib.hipsim_null_stream_reset()

    def offenders():
        return int(sim_lib.hipsim_null_stream_ops()), sim_lib.hipsim_null_stream_first().decode()
    return offenders


@pytest.mark.parametrize("family", sorted(S.FAMILIES))
def test_no_operation_on_the_null_stream(sim_session, audit, monkeypatch, family):
    S.FAMILIES[family](sim_session, monkeypatch)
    n, first = audit()
    assert n == 0, f"{family}: {n} operations on the null stream, the first: {first}"


def test_context_level_on_one_simulated_gpu(sim_lib, audit):
    """urcco_context_build_device on one simulated GPU (test_sim_context.context_reuse_case: three builds, twice each, in stream-per-event and single-stream
    mode).  The context owns its streams and creates each of them, so its count is zero as well: the simulator passes no input stream (a NULL input stream
    means "the inputs are ready", and then the context records and waits for nothing on it), and the one-session reference driver inside the case runs on
    its session's own stream."""
    from test_sim_context import context_reuse_case
    context_reuse_case(sim_lib, torch.device("cpu"))
    n, first = audit()
    assert n == 0, f"context level: {n} operations on the null stream, the first: {first}"


class _HostStream:
    """the simulator executes synchronously: nothing is ever pending, and there is nothing to wait for"""

    def synchronize(self):
        pass

    def query(self):
        return False


@pytest.mark.parametrize("name", sorted(S.PROTOCOL))
def test_protocol_problems(sim_session, audit, monkeypatch, name):
    """The stale-data protocol of tests/test_gpu_streams.py with the simulator in the GPU's place: its problem pairs are well formed (equal sizes, different
    references -- CallSet asserts both), the call gives ref(A) on A and ref(B) after B was copied over A in place, and nothing ran on the null stream.  The
    simulator cannot show stale data; this keeps the protocol's own code honest where there is no GPU."""
    S.run_protocol(S.PROTOCOL[name](sim_session, monkeypatch), sim_session, _HostStream(), lambda: None, log=lambda line: None)
    n, first = audit()
    assert n == 0, f"{name}: {n} operations on the null stream, the first: {first}"
