"""The session level on a caller's non-blocking stream on the MI355X.  Every other GPU test binds its session to torch's current stream at the time, the
null stream: urcco_session_create then makes a blocking stream of its own, and whatever the library or the Python layer leaves on the wrong stream is still
ordered by the null stream's implicit barrier.  Here the session is bound to `side = torch.cuda.Stream()` -- created with hipStreamNonBlocking, so nothing
is ordered with it but what is enqueued on it -- and every test body runs inside `with torch.cuda.stream(side)`: the contract a caller keeps (the
DeviceSession docstring).

(a) Coherence: one existing case per family (tests/stream_cases.py FAMILIES, the list tests/test_sim_streams.py audits), with its own reference and its
    own exact comparison.
(b) The stale-data protocol (stream_cases.run_protocol) per call set: problem A is run and checked; then a delay of DELAY_MS, device-to-device copies of a
    problem B of the same sizes over A's inputs and the same call are enqueued on `side`, and the result must be ref(B) bit for bit.  An operation that
    the library or the Python layer issued on another stream does not wait for the delay: it reads A, or scratch of A's run, all of it valid and in range
    for B, and the result shows it.  For the call sets that do not synchronise -- recommend, recommend_driven, history_append + history_trim -- `side` must
    still be busy when the call returns: the whole enqueue happened under the delay.  The others synchronise by design, and the protocol covers what
    they enqueue before that: urcco_dev_audience and urcco_dev_quota_cut wait once for their plan -- an audience call is a phase of its own, so the
    second chunk's call gets a delay and B of its own (audience_second_chunk); quota_cut's launches behind its plan cannot be entered separately --, and
    the user_recommendations chain (history_rows, recommend, explain through the Python function) waits in history_rows for the bound totals
    (DeviceSession._bounded_rows): the Python layer's torch ops in front of it and the bounds call run under the delay, the rows call, recommend and
    explain behind the read do not.  That second phase of history_rows / item_rows / props_rows cannot be given B on its own -- it writes into
    capacities sized by the totals of the inputs its first phase saw, so other inputs could leave a buffer -- and is not covered; nor is a call whose
    arena grows (every call set runs once before the delay, so the arena has its size).
(c) The control: the same call through a second session bound to another non-blocking stream, made while the delay and the copies of B are still queued on
    `side`, reads A and gives ref(A), not ref(B): the protocol can fail.  Stale but valid data by construction.
The session is closed at the end of the module and `side` used once more: the library must not destroy a stream it does not own."""
import pytest
import torch

import stream_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def side_session():
    from universal_recommender_amd import _lib
    from universal_recommender_amd.device import DeviceSession
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    import __graft_entry__
    __graft_entry__.build_hip()   # no-op when the in-tree liburcco.so is newer than its sources
    side = torch.cuda.Stream()
    s = DeviceSession(torch.device("cuda", 0), _lib.load(_lib.DEFAULT_PATH), stream=side)
    assert s.torch_stream is side and side.cuda_stream != 0
    yield s, side
    s.close()
    with torch.cuda.stream(side):   # the library did not own the stream: it is still there, and usable
        total = torch.arange(1024, device="cuda").sum()
    side.synchronize()
    assert int(total) == 1023 * 512


@pytest.fixture(autouse=True)
def on_side(side_session):
    with torch.cuda.stream(side_session[1]):
        yield


@pytest.fixture(scope="module")
def delay(side_session):
    """-> a function that enqueues DELAY_MS of device time on `side`: torch.cuda._sleep, its cycles calibrated here with two events (one large sort per
    few milliseconds where this torch has no _sleep)"""
    _, side = side_session
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        if hasattr(torch.cuda, "_sleep"):
            unit, work = 10_000_000, torch.cuda._sleep
        else:
            keys = torch.rand(1 << 24, device="cuda")
            unit, work = 1, lambda n: [torch.sort(keys) for _ in range(n)]
        work(unit)
        e0.record(side)
        work(unit)
        e1.record(side)
        e1.synchronize()
    ms = e0.elapsed_time(e1)
    n = max(int(unit * S.DELAY_MS / ms) + 1, 1)
    print(f"stream contract: delay of {S.DELAY_MS} ms = {n} {'cycles of torch.cuda._sleep' if unit > 1 else 'sorts of 2^24 keys'} ({unit} took {ms:.3f} ms)")
    return lambda: work(n)


@pytest.mark.parametrize("family", sorted(S.FAMILIES))
def test_coherence(side_session, monkeypatch, family):
    S.FAMILIES[family](side_session[0], monkeypatch)


@pytest.mark.parametrize("name", sorted(S.PROTOCOL))
def test_stale_data_protocol(side_session, delay, monkeypatch, name):
    sess, side = side_session
    S.run_protocol(S.PROTOCOL[name](sess, monkeypatch), sess, side, delay)


def test_control_a_call_on_another_stream_reads_the_old_inputs(side_session, delay, monkeypatch):
    from universal_recommender_amd.device import DeviceSession
    sess, side = side_session
    other = torch.cuda.Stream()
    cs = S.PROTOCOL["recommend"](sess, monkeypatch)
    s2 = DeviceSession(sess.device, sess.lib, stream=other)
    try:
        side.synchronize()                                       # A is on the device
        with torch.cuda.stream(other):                           # once before the delay: the second session's arena and torch's pool of `other` have their size
            cs.compare(S.host(cs.call(s2)), cs.want_a)
        delay()
        cs.load(cs.b)                                            # queued on `side`, behind the delay
        with torch.cuda.stream(other):
            out = cs.call(s2)
            other.synchronize()
            pending = side.query() is False
            got = S.host(out)
        assert pending, "the delay ran out before the call on the other stream finished: the control proves nothing"
        cs.compare(got, cs.want_a)
        with pytest.raises(AssertionError):
            cs.compare(got, cs.want_b)
        side.synchronize()
        cs.compare(S.host(cs.call(sess)), cs.want_b)             # and on `side` itself the inputs are B now
    finally:
        cs.load(cs.a)
        side.synchronize()
        s2.close()
