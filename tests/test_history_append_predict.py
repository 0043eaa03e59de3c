"""DeviceHistory.append / append_dict (decision D21): a history that was loaded in part and appended to gives batch_predict, user_recommendations and
evaluate exactly what a history built from the whole streams gives -- the handmade golden's model (tests/golden/handmade.json) on the simulator session,
one user the first load never saw, plain scoring and term_weights="idf"; the streams form with times and a growing user id space; the ValueErrors
of append, each of which leaves the history as it was."""
import numpy as np
import pytest
import torch

import history_append_cases as A
import history_ref as H


def halves(history, unseen):
    """(first, rest): the first half of every list of every user but `unseen`, and what remains -- `unseen` whole"""
    first = {u: {ev: ids[: len(ids) // 2] for ev, ids in evs.items()} for u, evs in history.items() if u != unseen}
    rest = {u: {ev: ids[len(ids) // 2:] if u != unseen else ids for ev, ids in evs.items()} for u, evs in history.items()}
    return first, rest


def test_append_dict_gives_from_dicts_answers(sim_session):
    from universal_recommender_amd.history import DeviceHistory
    algo, model, history, items = A.handmade_stack(sim_session, 3)
    unseen = list(history)[1]
    first, rest = halves(history, unseen)
    assert unseen not in first and any(len(ids) > 1 for evs in first.values() for ids in evs.values())
    dh = DeviceHistory.from_dict(sim_session, model, first)
    assert dh.user_index(unseen) == -1
    n_before = dh.n_users
    assert dh.append_dict(model, rest) is dh
    assert dh.n_users == n_before + 1 and dh.user_index(unseen) == n_before and dh.user_index("heavy") >= 0
    whole = DeviceHistory.from_dict(sim_session, model, history)
    assert set(dh.types) == set(whole.types) and all(dh.types[ev].n_events == whole.types[ev].n_events for ev in whole.types)
    qs = A.handmade_queries(history, items)
    for weights in (None, "idf"):
        for blacklist in (None, [], ["purchase", "view"]):
            algo.ap.blacklistEvents = blacklist
            want = algo.batch_predict(model, qs, whole, term_weights=weights)
            got = algo.batch_predict(model, qs, dh, term_weights=weights)
            assert got == want == algo.batch_predict(model, qs, history, term_weights=weights), (weights, blacklist)
            assert any(s["score"] > 0 for r in want for s in r["itemScores"])
    algo.ap.blacklistEvents = None
    # a second append, of events alone (every user is known), and a history of integer ids refuses the dict form
    more = {"heavy": {"view": [items[0], items[1]]}, unseen: {"purchase": [items[2]]}}
    both = {u: {ev: ids + more.get(u, {}).get(ev, []) for ev, ids in evs.items()} for u, evs in history.items()}
    dh.append_dict(model, more)
    assert algo.batch_predict(model, qs, dh) == algo.batch_predict(model, qs, both)
    with pytest.raises(ValueError):
        DeviceHistory.from_streams(sim_session, model, {}, n_users=3).append_dict(model, more)


def _device(sess, streams, lo=None, hi=None):
    return {ev: tuple(torch.from_numpy(a[lo:hi]).to(sess.device) if a is not None else None for a in st) for ev, st in streams.items()}


def _state(dh):
    return (dh.n_users, dh.user_ids, {ev: (st.n_events, st.items.data_ptr(), st.idx_row_ptr.data_ptr(), st.idx_pos.data_ptr(), st.idx_row_ptr.clone(),
                                           st.items.clone()) for ev, st in dh.types.items()})


def _same_state(a, b):
    return a[:2] == b[:2] and a[2].keys() == b[2].keys() and all(x[:4] == y[:4] and torch.equal(x[4], y[4]) and torch.equal(x[5], y[5])
                                                                for x, y in zip(a[2].values(), b[2].values()))


def test_append_streams_gives_from_streams_answers(sim_session):
    """Streams with times (negative ones, ties) and without; three appends, the id space grows with the second; an event type that arrives later;
    an event type without new events whose index is only extended.  batch_predict, user_recommendations and evaluate against from_streams of the whole."""
    from universal_recommender_amd.history import GROWTH, DeviceHistory
    n_users = 60
    algo, model = H.predict_stack(sim_session, 400, 60, 40)
    streams, history = H.make_stream_history(41, n_users, 60, 40)
    # the events of the users below 40 first, as far as half of each stream; "view" only from the second append on
    cut = {ev: st[0].size // 2 for ev, st in streams.items()}
    early = {ev: tuple(a[: cut[ev]][st[0][: cut[ev]] < 40] if a is not None else None for a in st) for ev, st in streams.items()}
    late = {ev: tuple(np.concatenate([a[: cut[ev]][st[0][: cut[ev]] >= 40], a[cut[ev]:]]) if a is not None else None for a in st) for ev, st in streams.items()}
    joined = {ev: tuple(np.concatenate([a, b]) if a is not None else None for a, b in zip(early[ev], late[ev])) for ev in streams}
    whole = DeviceHistory.from_streams(sim_session, model, _device(sim_session, joined), n_users=n_users)
    dh = DeviceHistory.from_streams(sim_session, model, {"purchase": _device(sim_session, early)["purchase"]}, n_users=40)
    assert dh.append({"view": _device(sim_session, early)["view"]}) is dh and dh.n_users == 40 and set(dh.types) == {"purchase", "view"}
    third = {ev: st[0].size // 3 for ev, st in late.items()}
    dh.append({"purchase": _device(sim_session, late, 0, third["purchase"])["purchase"]})                  # the default n_users: the largest id + 1
    assert dh.n_users == int(late["purchase"][0][: third["purchase"]].max()) + 1 and dh.types["view"].idx_row_ptr.numel() == dh.n_users + 1
    dh.append({ev: tuple(None if a is None else a[third[ev] if ev == "purchase" else 0:] for a in st) for ev, st in _device(sim_session, late).items()}, n_users=n_users)
    assert dh.n_users == n_users
    for ev, st in dh.types.items():
        w = whole.types[ev]
        assert st.n_events == w.n_events and torch.equal(st.items, w.items) and (st.times is None) == (w.times is None) and torch.equal(st.idx_row_ptr, w.idx_row_ptr)
        assert st.items.numel() == st.n_events and st.idx_pos.numel() == st.n_events and st.items_buf.numel() >= st.n_events
        assert st.times is None or torch.equal(st.times, w.times)
    pos = dh.types["purchase"]
    assert pos.idx_spare is not None and pos.idx_spare[1].data_ptr() != pos.idx_buf[1].data_ptr() and GROWTH == 2
    us = list(range(n_users))
    qs = [{"user": u} for u in us] + [{"user": u, "item": int(u * 2) % 60} for u in us[1::7]] + [{"user": u, "userBias": -1.0, "num": 5} for u in us[2::5]]
    qs += [{"user": n_users + 100}, {}, {"item": 5}]
    for blacklist in (None, ["purchase", "view"]):
        algo.ap.blacklistEvents = blacklist
        want = algo.batch_predict(model, qs, whole)
        assert algo.batch_predict(model, qs, dh) == want == algo.batch_predict(model, qs, history)
        assert all(torch.equal(a, b) for a, b in zip(algo.user_recommendations(model, dh), algo.user_recommendations(model, whole)))
    algo.ap.blacklistEvents = None
    assert any(s["score"] > 0 for r in want for s in r["itemScores"])
    # hold-out evaluation, the views as the training side (a user's own purchases are never recommended back): an appended history as the training
    # side and as the truth side
    dev_early, dev_late, dev_joined = (_device(sim_session, x) for x in (early, late, joined))
    train = DeviceHistory.from_streams(sim_session, model, {"view": dev_joined["view"]}, n_users=n_users)
    train_appended = DeviceHistory.from_streams(sim_session, model, {"view": dev_early["view"]}, n_users=40).append({"view": dev_late["view"]}, n_users=n_users)
    want = algo.evaluate(model, train, whole, ks=(1, 5), num=10)
    assert want["evaluated"] > 0 and any(want["hit_rate"])
    for got in (algo.evaluate(model, train_appended, whole, ks=(1, 5), num=10), algo.evaluate(model, train, dh, ks=(1, 5), num=10)):
        assert {k: v for k, v in got.items() if k != "per_user"} == {k: v for k, v in want.items() if k != "per_user"}
        assert all(torch.equal(got["per_user"][k], want["per_user"][k]) for k in ("hits", "ap", "ndcg"))


def test_append_refuses_and_leaves_the_history_unchanged(sim_session):
    from universal_recommender_amd.history import DeviceHistory, _Stream
    algo, model = H.predict_stack(sim_session, 400, 60, 40)
    streams, _ = H.make_stream_history(41, 60, 60, 40)
    dev = _device(sim_session, streams)
    dh = DeviceHistory.from_streams(sim_session, model, dev, n_users=60)
    before = _state(dh)
    (u, i, t), (vu, vi, _) = dev["purchase"], dev["view"]
    good = (u[:5], i[:5], t[:5])
    bad = [{"purchase": (u.to(torch.int64), i, t)}, {"purchase": (u, i.to(torch.int64), t)}, {"purchase": (u[:-1], i, t)}, {"purchase": (u, i, t.to(torch.int32))},
           {"purchase": (u, i, t[:-1])}, {"purchase": (u, i[:-1], None)},
           {"purchase": (u, i, None)},                                       # times missing for a stream that has them
           {"view": (vu, vi, t[: vu.numel()])},                              # times given for a stream that has none
           {"purchase": good, "view": (vu, vi[:-1], None)}]                  # the first stream is fine, the second is not: neither is appended
    for streams_bad in bad:
        with pytest.raises(ValueError):
            dh.append(streams_bad)
        assert _same_state(_state(dh), before)
    with pytest.raises(ValueError):
        dh.append({"purchase": good}, n_users=59)                            # a shrinking n_users
    with pytest.raises(ValueError):
        dh.append({"purchase": good}, user_ids={k: k for k in range(7)})     # ... by way of a smaller user_ids
    with pytest.raises(ValueError):
        DeviceHistory(sim_session, 60, None, dict(dh.types)).append({"new event": (vu, vi, None)})    # a new event name, no model to take its columns from
    assert _same_state(_state(dh), before)
    p = dh.types["purchase"]                                                 # a stream built by hand without its number of events: no append, no extension
    hand = DeviceHistory(sim_session, 60, None, {"purchase": _Stream(p.n_cols, p.idx_row_ptr, p.idx_pos, p.items, p.times, p.col_map)}, model)
    for streams_bad, n in (({"purchase": good}, None), ({}, 61)):
        with pytest.raises(ValueError):
            hand.append(streams_bad, n_users=n)
    assert hand.append({}) is hand and hand.types["purchase"].idx_row_ptr is p.idx_row_ptr
    assert dh.append({}) is dh and _same_state(_state(dh), before)           # nothing to do: no call, no change
    dh.append({"purchase": good})
    assert dh.types["purchase"].n_events == before[2]["purchase"][0] + 5 and dh.types["view"].idx_row_ptr.data_ptr() == before[2]["view"][2]
