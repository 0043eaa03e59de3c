"""The whole stack -- DataSource -> Preparator -> URAlgorithm.train -> DeviceModel -> batch_predict -- against the reference's integration
goldens (tests/golden/handmade.json, item_sets.json).  The goldens hold Elasticsearch scores; what they pin is WHICH items get a positive
score (tests/membership.py), and that is what batch_predict must reproduce with its own score."""
import json
import os

import pytest
import torch

from membership import handmade_dates, positive_items, item_properties

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    doc = json.load(open(os.path.join(GOLDEN, name)))
    history, items = {}, []
    for u, e, i in doc["events"]:
        history.setdefault(u, {}).setdefault(e, []).append(i)     # the UNFILTERED event stream, oldest first
        if i not in items:
            items.append(i)
    return doc, history, items


def _stack(name, sess):
    """(algorithm, device model, model as item -> {event: [ids]}, history, all items, golden document)."""
    from universal_recommender_amd.data_source import DataSource, DataSourceParams
    from universal_recommender_amd.preparator import Preparator
    from universal_recommender_amd.recommend import DeviceModel
    from universal_recommender_amd.ur_algorithm import URAlgorithm, URAlgorithmParams, toStringMap
    doc, history, items = _load(name)
    lines = [",".join(e) for e in doc["events"]] + [f"{i},$set,{p}" for i, p in doc["sets"]]
    engine = {"datasource": {"params": doc["datasource_params"]}, "algorithms": [{"name": "ur", "params": doc["algorithm_params"]}]}
    td = DataSource(DataSourceParams.from_engine_json(engine)).readTraining(lines)
    ap = URAlgorithmParams.from_engine_json(engine)
    ap.seed = 1
    algo = URAlgorithm(ap, device=0, library=sess.lib)
    trained = algo.train(Preparator().prepare(td))
    docs = {}
    for ev, ind in trained.coocurrenceMatrices:
        for item, m in toStringMap(ind, ev).items():
            docs.setdefault(item, {}).update(m)
    return algo, DeviceModel.from_indicators(sess, trained.coocurrenceMatrices), docs, history, items, doc


def _accept(doc, q, pos, cands):
    """The acceptance rule of the golden reader (tests/test_golden_reference.py, _check_queries), restated: `pos` = the items this stack gives
    a positive score, `cands` = the items that pass the query's must / must_not clauses."""
    num = q["query"].get("num", doc["algorithm_params"].get("num", 20))
    start = q["query"].get("from", 0)
    expected_pos = [s["item"] for s in q["itemScores"] if s["score"] > 0]
    expected_all = [s["item"] for s in q["itemScores"]]
    good = set(expected_all) <= set(cands)
    if len(pos) <= start:
        good &= expected_pos == []
    elif len(pos) - start <= num:
        good &= set(expected_pos) == set(pos) if start == 0 else set(expected_pos) <= set(pos)
    else:
        good &= len(expected_pos) == num and set(expected_pos) <= set(pos)
    return good


def _handmade(sess):
    algo, model, docs, history, items, doc = _stack("handmade.json", sess)
    dates = handmade_dates()
    mask = {item: d["available"] <= 0.0 <= d["expires"] for item, d in dates.items()}
    props = item_properties(doc["sets"])
    plain = [q for q in doc["queries"] if "fields" not in q["query"] and "dateRange" not in q["query"]]
    assert len(doc["queries"]) == 28 and len(plain) == 18
    in_model = [model.item_name(i) for i in range(model.n_items)]
    # num = every item: the positive set is the one the membership rule derives from the model
    wide = algo.batch_predict(model, [{k: v for k, v in q["query"].items() if k not in ("num", "from")} | {"num": model.n_items} for q in plain], history, mask)
    positives = []
    for q, res in zip(plain, wide):
        cands, pos = positive_items(q["query"], docs, items, history, props, "purchase", dates)
        got = res["itemScores"]
        assert {s["item"] for s in got if s["score"] > 0} == set(pos) & set(in_model), q["title"]
        assert set(pos) <= set(in_model), "a positive item outside the primary's item dictionary"
        assert {s["item"] for s in got} <= set(cands), q["title"]
        scores = [s["score"] for s in got]
        assert scores == sorted(scores, reverse=True)
        positives.append(([s["item"] for s in got if s["score"] > 0], cands))
    # the golden's own num / from
    for q, res, (pos, cands) in zip(plain, algo.batch_predict(model, [q["query"] for q in plain], history, mask), positives):
        mine = [s["item"] for s in res["itemScores"] if s["score"] > 0]
        assert _accept(doc, q, pos, cands), q["title"]
        num, start = q["query"].get("num", doc["algorithm_params"].get("num", 20)), q["query"].get("from", 0)
        assert len(res["itemScores"]) <= num and set(mine) <= set(pos)
        assert len(mine) == max(0, min(len(pos) - start, num)), q["title"]
        expected_pos = [s["item"] for s in q["itemScores"] if s["score"] > 0]
        if start == 0 and len(pos) <= num:
            assert set(mine) == set(expected_pos), q["title"]
        one = algo.predict(model, q["query"], history, mask)
        assert one == res
    # negative control: without the exclusion list a user query returns an item the golden never shows
    algo.ap.blacklistEvents = []
    try:
        user_q = [q for q in plain if set(q["query"]) == {"user"}]
        leaked = 0
        for q, res in zip(user_q, algo.batch_predict(model, [q["query"] for q in user_q], history, mask)):
            leaked += bool({s["item"] for s in res["itemScores"]} - {s["item"] for s in q["itemScores"]})
        assert user_q and leaked >= 1
    finally:
        algo.ap.blacklistEvents = None
    # what is deliberately left out says so
    rest = [q for q in doc["queries"] if q not in plain]
    assert len(rest) == 10
    for q in rest:
        with pytest.raises(NotImplementedError, match="fields|dateRange"):
            algo.batch_predict(model, [q["query"]], history, mask)
    for key in ("userBias", "itemBias"):
        with pytest.raises(NotImplementedError, match=key):
            algo.predict(model, {"user": "u1", key: -1.0}, history)
    with pytest.raises(ValueError):
        algo.predict(model, {"user": "u1", "num": 200, "from": 100}, history)


def _item_sets(sess):
    algo, model, docs, history, items, doc = _stack("item_sets.json", sess)
    assert algo.recsModel == "collabFiltering" and len(doc["queries"]) == 7
    res = algo.batch_predict(model, [q["query"] for q in doc["queries"]], history)
    for q, r in zip(doc["queries"], res):
        assert {s["item"] for s in r["itemScores"]} == {s["item"] for s in q["itemScores"]}, q["title"]
        assert all(s["score"] > 0 for s in r["itemScores"])
    empty = [r for q, r in zip(doc["queries"], res) if q["query"]["itemSet"] == ["iPhone 6p"]]
    assert empty and empty[0]["itemScores"] == []


def test_handmade_queries_on_the_simulator(sim_session):
    _handmade(sim_session)


def test_item_set_queries_on_the_simulator(sim_session):
    _item_sets(sim_session)


@pytest.mark.gpu
def test_handmade_queries_on_the_gpu(gpu_session):
    _handmade(gpu_session)


@pytest.mark.gpu
def test_item_set_queries_on_the_gpu(gpu_session):
    _item_sets(gpu_session)
