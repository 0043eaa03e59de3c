"""batch_predict with the user history resident on the device (history.DeviceHistory, decision D17) returns exactly the items and scores it
returns with the dict form of `history`: the handmade fixture of tests/test_recommend_golden.py plus a synthetic user with more events than
maxItemsPerUser, on the simulator session; and DeviceHistory.from_streams with real times (negative ones, ties) against the dict sorted on the host."""
import pytest

import history_ref as H

from test_recommend_golden import _load

HEAVY = 520      # events of the synthetic user: more than the default maxItemsPerUser (500)


def stack(sess, cap=None):
    from universal_recommender_amd.data_source import DataSource, DataSourceParams
    from universal_recommender_amd.preparator import Preparator
    from universal_recommender_amd.recommend import DeviceModel
    from universal_recommender_amd.ur_algorithm import URAlgorithm, URAlgorithmParams
    doc, history, items = _load("handmade.json")
    lines = [",".join(e) for e in doc["events"]] + [f"{i},$set,{p}" for i, p in doc["sets"]]
    engine = {"datasource": {"params": doc["datasource_params"]}, "algorithms": [{"name": "ur", "params": doc["algorithm_params"]}]}
    td = DataSource(DataSourceParams.from_engine_json(engine)).readTraining(lines)
    ap = URAlgorithmParams.from_engine_json(engine)
    ap.seed = 1
    algo = URAlgorithm(ap, device=0, library=sess.lib)
    trained = algo.train(Preparator().prepare(td))
    model = DeviceModel.from_indicators(sess, trained.coocurrenceMatrices, properties={})      # {}: serves the negative biases
    if cap is not None:
        for ind in ap.indicators:
            ind.maxItemsPerUser = cap
    # the event store also knows a user the model never saw: old purchases that fall out of the window of the most recent ones, an item id
    # no dictionary holds, views in between
    purchases = [i for _, e, i in doc["events"] if e == "purchase"]
    recent = sorted(set(purchases))[:2]
    old = [i for i in dict.fromkeys(purchases) if i not in recent][:3]
    assert len(old) == 3
    history["heavy"] = {"purchase": old + ["no such item"] + [recent[k % 2] for k in range(HEAVY - 4)], "view": [i for _, e, i in doc["events"] if e == "view"][:7] + ["nothing"]}
    return algo, model, history, items, old, recent


def queries(history, items):
    users = list(history) + ["nobody"]
    qs = [{"user": u} for u in users]
    qs += [{"user": u, "item": items[k % len(items)]} for k, u in enumerate(users)]
    qs += [{"user": u, "userBias": -1.0} for u in users[:4] + ["heavy", "nobody"]]
    qs += [{"user": u, "userBias": 2.5, "blacklistItems": items[k:k + 2]} for k, u in enumerate(users)]
    qs += [{"user": "heavy", "from": f, "num": n} for f, n in ((0, 2), (1, 3), (2, 20))]
    qs += [{"user": u, "eventNames": ["view", "purchase"]} for u in users[:3] + ["heavy"]]
    qs += [{"user": u, "eventNames": ["category-pref"], "num": 6} for u in users[:3]]
    qs += [{}, {"item": items[0]}, {"itemSet": items[:2]}, {"user": "heavy", "itemSet": items[1:3], "returnSelf": True, "item": items[2]}]
    return qs


@pytest.mark.parametrize("cap", [None, 3])
def test_device_history_gives_the_dicts_answers(sim_session, cap):
    from universal_recommender_amd.history import DeviceHistory
    algo, model, history, items, old, recent = stack(sim_session, cap)
    dh = DeviceHistory.from_dict(sim_session, model, history)
    assert dh.user_index("heavy") >= 0 and dh.user_index("nobody") == -1 and set(dh.types) == {"purchase", "view", "category-pref"}
    qs = queries(history, items)
    for blacklist in (None, [], ["purchase", "view"]):
        algo.ap.blacklistEvents = blacklist
        want = algo.batch_predict(model, qs, history)
        got = algo.batch_predict(model, qs, dh)
        assert len(want) == len(qs)
        for q, w, g in zip(qs, want, got):
            assert g == w, (blacklist, q, g, w)          # items AND scores, exactly
        assert algo.predict(model, {"user": "heavy"}, dh) == want[qs.index({"user": "heavy"})]
        assert any(r["itemScores"] for r in want) and any(s["score"] > 0 for r in want for s in r["itemScores"])
    algo.ap.blacklistEvents = None
    # the cap is at work: the heavy user's old purchases are outside the window -- dropping them from the history changes no user-history score,
    # but they stay excluded (the exclusions have no cap)
    res = algo.predict(model, {"user": "heavy", "num": len(items)}, dh)
    assert not {s["item"] for s in res["itemScores"]} & set(old + recent)
    trimmed = dict(history, heavy=dict(history["heavy"], purchase=history["heavy"]["purchase"][4:]))
    res_trimmed = algo.predict(model, {"user": "heavy", "num": len(items)}, DeviceHistory.from_dict(sim_session, model, trimmed))
    scores = {s["item"]: s["score"] for s in res["itemScores"]}
    assert all(scores[s["item"]] == s["score"] for s in res_trimmed["itemScores"] if s["item"] in scores)
    assert {s["item"] for s in res_trimmed["itemScores"]} - set(scores) <= set(old)


def test_from_streams_gives_the_dicts_answers(sim_session):
    """Integer user ids, shuffled events, int64 times from the key families of tests/history_ref.py, one event type without times; caps 6 and 70 against
    0..150 events per user; users resolved by a dict and by their integer id; the ValueErrors of from_streams."""
    algo, model = H.predict_stack(sim_session, 400, 60, 40)
    streams, history = H.make_stream_history(41, 60, 60, 40)
    H.check_from_streams(sim_session, algo, model, 60, streams, history)
