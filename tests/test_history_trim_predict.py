"""DeviceHistory.trim (decision D22): a history that was trimmed -- events older than a cut-off gone, some users deleted -- gives batch_predict,
user_recommendations and evaluate exactly what a history built by from_streams from the filtered whole streams gives, with the same n_users; so does
an append onto it.  On the simulator session, a device-built model over integer ids; a timed stream ("purchase": negative times, ties) and an untimed
one ("view"); the ValueErrors of trim, each of which leaves the history as it was; last_trim and the buffers' capacities."""
import numpy as np
import pytest
import torch

import history_ref as H

N_USERS = 60
DROP = [3, 10, 0, 41]


def _device(sess, streams, lo=None, hi=None):
    return {ev: tuple(torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(sess.device) if a is not None else None for a in st) for ev, st in streams.items()}


def _filtered(streams, cut, drop, events=("purchase",)):
    """the streams without the events of the users in `drop` and, for the timed types in `events`, without those older than cut"""
    out = {}
    for ev, (u, i, t) in streams.items():
        keep = ~np.isin(u, drop)
        if t is not None and ev in events and cut is not None:
            keep &= t >= cut
        out[ev] = (u[keep], i[keep], t[keep] if t is not None else None)
    return out


def _queries():
    us = list(range(N_USERS))
    qs = [{"user": u} for u in us] + [{"user": u, "item": int(u * 2) % 60} for u in us[1::7]] + [{"user": u, "userBias": -1.0, "num": 5} for u in us[2::5]]
    return qs + [{"user": N_USERS + 100}, {}, {"item": 5}]


def _same_answers(algo, model, got_h, want_h):
    qs = _queries()
    for weights in (None, "idf"):
        for blacklist in (None, ["purchase", "view"]):
            algo.ap.blacklistEvents = blacklist
            want = algo.batch_predict(model, qs, want_h, term_weights=weights)
            assert algo.batch_predict(model, qs, got_h, term_weights=weights) == want, (weights, blacklist)
            assert any(s["score"] > 0 for r in want for s in r["itemScores"])
        assert all(torch.equal(a, b) for a, b in zip(algo.user_recommendations(model, got_h), algo.user_recommendations(model, want_h)))
    algo.ap.blacklistEvents = None


def _same_evaluation(algo, model, train_a, truth_a, train_b, truth_b):
    got, want = algo.evaluate(model, train_a, truth_a, ks=(1, 5), num=10), algo.evaluate(model, train_b, truth_b, ks=(1, 5), num=10)
    assert want["evaluated"] > 0 and any(want["hit_rate"])
    assert {k: v for k, v in got.items() if k != "per_user"} == {k: v for k, v in want.items() if k != "per_user"}
    assert all(torch.equal(got["per_user"][k], want["per_user"][k]) for k in ("hits", "ap", "ndcg"))


@pytest.fixture(scope="module")
def stack(sim_session):
    algo, model = H.predict_stack(sim_session, 400, 60, 40)
    streams, _ = H.make_stream_history(41, N_USERS, 60, 40)
    cut = int(np.sort(streams["purchase"][2])[streams["purchase"][2].size // 2])      # an element of the stream: events with time == cut exist
    return algo, model, streams, cut


def _state(dh):
    return (dh.n_users, dh.user_ids, {ev: (st.n_events, st.items.data_ptr(), st.idx_row_ptr.data_ptr(), st.idx_pos.data_ptr(), st.idx_row_ptr.clone(), st.items.clone())
                                      for ev, st in dh.types.items()})


def _same_state(a, b):
    return a[:2] == b[:2] and a[2].keys() == b[2].keys() and all(x[:4] == y[:4] and torch.equal(x[4], y[4]) and torch.equal(x[5], y[5])
                                                                for x, y in zip(a[2].values(), b[2].values()))


def test_trim_gives_from_streams_answers(sim_session, stack):
    from universal_recommender_amd.history import DeviceHistory
    algo, model, streams, cut = stack
    t = streams["purchase"][2]
    assert (t < 0).any() and 0.3 < np.mean(t < cut) < 0.7 and (t == cut).any()
    dh = DeviceHistory.from_streams(sim_session, model, _device(sim_session, streams), n_users=N_USERS)
    before = {ev: st.n_events for ev, st in dh.types.items()}
    assert dh.trim(before_ms=cut, drop_users=DROP + [N_USERS + 7, "nobody"]) is dh
    want = _filtered(streams, cut, DROP)
    whole = DeviceHistory.from_streams(sim_session, model, _device(sim_session, want), n_users=N_USERS)
    assert dh.n_users == N_USERS and dh.last_trim == {ev: (before[ev], want[ev][0].size) for ev in streams}
    assert all(0 < want[ev][0].size < before[ev] for ev in streams)
    for ev, st in dh.types.items():
        w = whole.types[ev]
        assert st.n_events == w.n_events == st.items.numel() == st.idx_pos.numel() and torch.equal(st.items, w.items) and torch.equal(st.idx_row_ptr, w.idx_row_ptr)
        assert (st.times is None) == (w.times is None) and (st.times is None or torch.equal(st.times, w.times))
        assert st.items_buf.numel() == before[ev] and (st.times is None or st.times_buf.numel() == before[ev])      # the old capacity: room for the next append
    _same_answers(algo, model, dh, whole)
    train = DeviceHistory.from_streams(sim_session, model, {"view": _device(sim_session, streams)["view"]}, n_users=N_USERS)
    _same_evaluation(algo, model, train, dh, train, whole)
    train_want = DeviceHistory.from_streams(sim_session, model, {"view": _device(sim_session, want)["view"]}, n_users=N_USERS)
    _same_evaluation(algo, model, train.trim(drop_users=torch.tensor(DROP, dtype=torch.int32)), whole, train_want, whole)


def test_append_onto_a_trimmed_history(sim_session, stack):
    """two thirds of every stream loaded, trimmed, the rest appended (into the capacity the trim left), trimmed again with a later cut-off"""
    from universal_recommender_amd.history import DeviceHistory
    algo, model, streams, cut = stack
    at = {ev: st[0].size * 2 // 3 for ev, st in streams.items()}
    first = {ev: tuple(a[: at[ev]] if a is not None else None for a in st) for ev, st in streams.items()}
    rest = {ev: tuple(a[at[ev]:] if a is not None else None for a in st) for ev, st in streams.items()}
    dh = DeviceHistory.from_streams(sim_session, model, _device(sim_session, first), n_users=N_USERS).trim(before_ms=cut, drop_users=DROP)
    caps = {ev: st.items_buf.numel() for ev, st in dh.types.items()}
    assert caps == at
    dh.append(_device(sim_session, rest))
    f = _filtered(first, cut, DROP)
    want = {ev: tuple(np.concatenate([a, b]) if a is not None else None for a, b in zip(f[ev], rest[ev])) for ev in streams}
    assert all(dh.types[ev].n_events == want[ev][0].size for ev in streams)
    assert any(dh.types[ev].items_buf.numel() == caps[ev] for ev in streams)          # an append that fitted the spare capacity allocated nothing
    whole = DeviceHistory.from_streams(sim_session, model, _device(sim_session, want), n_users=N_USERS)
    _same_answers(algo, model, dh, whole)
    later = int(np.sort(streams["purchase"][2])[streams["purchase"][2].size * 7 // 10])
    dh.trim(before_ms=later, drop_users=[5])
    whole = DeviceHistory.from_streams(sim_session, model, _device(sim_session, _filtered(want, later, [5])), n_users=N_USERS)
    assert all(torch.equal(dh.types[ev].items, whole.types[ev].items) and torch.equal(dh.types[ev].idx_row_ptr, whole.types[ev].idx_row_ptr) for ev in streams)
    _same_answers(algo, model, dh, whole)


def test_mixed_streams_and_refusals(sim_session, stack):
    from universal_recommender_amd.history import DeviceHistory, _Stream
    algo, model, streams, cut = stack
    dev = _device(sim_session, streams)
    dh = DeviceHistory.from_streams(sim_session, model, dev, n_users=N_USERS)
    before = _state(dh)
    for kw in (dict(before_ms=cut, events=["view"]), dict(before_ms=cut, events=["purchase", "view"]), dict(before_ms=cut, events=["no such event"]),
               dict(drop_users=[1], events=["no such event"]), dict(drop_users=torch.tensor([1], dtype=torch.int64))):
        with pytest.raises(ValueError):
            dh.trim(**kw)
        assert _same_state(_state(dh), before)
    assert dh.trim() is dh and dh.trim(drop_users=["nobody", N_USERS + 1]) is dh and dh.trim(drop_users=[]) is dh      # nothing to do: no call, no change
    assert _same_state(_state(dh), before) and dh.last_trim == {}
    p = dh.types["purchase"]                                   # a stream built by hand without its number of events is refused
    hand = DeviceHistory(sim_session, N_USERS, None, {"purchase": _Stream(p.n_cols, p.idx_row_ptr, p.idx_pos, p.items, p.times, p.col_map)}, model)
    with pytest.raises(ValueError):
        hand.trim(before_ms=cut)
    # before_ms alone: the timed stream only; the untimed one costs no call and keeps its tensors
    dh.trim(before_ms=cut)
    assert set(dh.last_trim) == {"purchase"} and dh.types["view"].items.data_ptr() == before[2]["view"][1] and dh.types["view"].n_events == before[2]["view"][0]
    whole = DeviceHistory.from_streams(sim_session, model, _device(sim_session, _filtered(streams, cut, [])), n_users=N_USERS)
    _same_answers(algo, model, dh, whole)
    dh.trim(before_ms=cut + 1, events=["purchase"])            # a named timed type
    assert set(dh.last_trim) == {"purchase"} and dh.last_trim["purchase"][1] < dh.last_trim["purchase"][0] == whole.types["purchase"].n_events
    # drop_users reaches every type, whatever `events` says
    dh.trim(drop_users=[7], events=["purchase"])
    assert set(dh.last_trim) == {"purchase", "view"}
    whole = DeviceHistory.from_streams(sim_session, model, _device(sim_session, _filtered(streams, cut + 1, [7])), n_users=N_USERS)
    _same_answers(algo, model, dh, whole)


def test_a_dropped_user_is_a_user_without_events(sim_session, stack):
    from universal_recommender_amd.history import DeviceHistory
    algo, model, streams, cut = stack
    names = {f"user-{u}": u for u in range(N_USERS)}
    dh = DeviceHistory.from_streams(sim_session, model, _device(sim_session, streams), user_ids=names)
    quiet = f"user-{N_USERS - 1}"                               # make_stream_history: the last two users own nothing
    was = algo.batch_predict(model, [{"user": "user-0"}, {"user": quiet}], dh)
    assert was[0] != was[1]
    dh.trim(drop_users=["user-0", "user-0", "somebody else"])
    assert dh.n_users == N_USERS and dh.user_ids is names and dh.user_index("user-0") == 0
    now = algo.batch_predict(model, [{"user": "user-0"}, {"user": quiet}, {"user": "user-1"}], dh)
    assert now[0] == now[1] == was[1]
    rp = dh.types["purchase"].idx_row_ptr
    assert int(rp[1]) == int(rp[0]) == 0 and int(rp[2]) > 0
    full = DeviceHistory.from_streams(sim_session, model, _device(sim_session, streams), user_ids=names)
    assert now[2] == algo.batch_predict(model, [{"user": "user-1"}], full)[0]
    # the capacity survives a trim of a buffer that an append grew
    n = full.types["view"].n_events
    u, i, _ = _device(sim_session, streams)["view"]
    full.append({"view": (u[:5], i[:5], None)})
    cap = full.types["view"].items_buf.numel()
    assert cap == 2 * n
    full.trim(drop_users=["user-2"])
    assert full.types["view"].items_buf.numel() == cap and full.last_trim["view"][0] == n + 5
