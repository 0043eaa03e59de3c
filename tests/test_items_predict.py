"""Item queries served from the device (decision D18): batch_predict(..., item_rows="device") returns exactly the items and scores of the host route,
with a dict history and with a DeviceHistory; similar_items returns, as device tensors, the rows batch_predict answers to {"item": x}; and
DeviceModel.indicator_row -- the host copy of the matrices -- is never touched on the device route.  On the simulator session: the handmade golden's
model with item properties and dates (rules, the available / expire rule), and a device-built model of 60 items over integer ids."""
import numpy as np
import pytest
import torch

import history_ref as H
from test_recommend_rules_golden import NOW_MS, _stack


@pytest.fixture(scope="module")
def handmade(sim_session):
    algo, model, _docs, history, items, *_ = _stack(sim_session)
    return algo, model, history, items


@pytest.fixture(scope="module")
def built(sim_session):
    return H.predict_stack(sim_session, 400, 60, 40)


def mixed_queries(history, items):
    users = list(history)
    cat = {"name": "categories", "values": ["Tablets", "Phones"]}
    qs = [{"item": i} for i in items] + [{"item": "no such item"}, {}, {"user": users[0]}]
    qs += [{"user": u, "item": items[k % len(items)]} for k, u in enumerate(users)]
    qs += [{"item": i, "fields": [dict(cat, bias=b)]} for i in items[:3] for b in (-1, 0, 2.5)]
    qs += [{"item": i, "itemBias": -1} for i in items] + [{"item": "no such item", "itemBias": -1}, {"user": users[1], "item": items[1], "itemBias": -1, "userBias": -1}]
    qs += [{"item": i, "itemBias": 3.0, "returnSelf": rs} for i in items[:4] for rs in (True, False)]
    qs += [{"item": items[2], "from": f, "num": n} for f, n in ((0, 2), (1, 3), (2, 20))]
    qs += [{"item": items[0], "blacklistItems": items[1:3]}, {"item": items[1], "itemSet": items[2:4]}, {"item": items[3], "eventNames": ["view"], "user": users[2]}]
    return qs


def with_max_query_events(algo, mqe):
    """maxQueryEvents is only read without per-indicator parameters (URAlgorithm.scala:203-211): drop them for the query side"""
    saved = (algo.ap.indicators, algo.ap.maxQueryEvents)
    if mqe is not None:
        algo.ap.indicators, algo.ap.maxQueryEvents = None, mqe
    return saved


@pytest.mark.parametrize("mqe", [None, 1])
def test_device_route_gives_the_host_routes_answers(handmade, mqe):
    algo, model, history, items = handmade
    qs = mixed_queries(history, items)
    saved = with_max_query_events(algo, mqe)
    try:
        want = algo.batch_predict(model, qs, history, now_ms=NOW_MS)
        got = algo.batch_predict(model, qs, history, now_ms=NOW_MS, item_rows="device")
        if mqe is not None:    # the cap is at work: some item's list is longer
            assert any(model.indicator_row(c, i).size > mqe for c in model.correlators for i in range(model.n_items))
    finally:
        algo.ap.indicators, algo.ap.maxQueryEvents = saved
    assert len(want) == len(qs)
    for q, w, g in zip(qs, want, got):
        assert g == w, (mqe, q, g, w)                    # items AND scores, exactly
    assert any(s["score"] > 0 for r in want for s in r["itemScores"])
    with pytest.raises(ValueError):
        algo.batch_predict(model, qs[:1], history, item_rows="gpu")


@pytest.mark.parametrize("mqe", [None, 1])
def test_device_route_with_a_device_history(sim_session, handmade, mqe):
    from universal_recommender_amd.history import DeviceHistory
    algo, model, history, items = handmade
    dh = DeviceHistory.from_dict(sim_session, model, history)
    qs = mixed_queries(history, items)
    saved = with_max_query_events(algo, mqe)
    try:
        want = algo.batch_predict(model, qs, dh, now_ms=NOW_MS)
        got = algo.batch_predict(model, qs, dh, now_ms=NOW_MS, item_rows="device")
        by_dict = algo.batch_predict(model, qs, history, now_ms=NOW_MS)
    finally:
        algo.ap.indicators, algo.ap.maxQueryEvents = saved
    for q, w, g, d in zip(qs, want, got, by_dict):
        assert g == w == d, (mqe, q, g, w, d)


@pytest.mark.parametrize("mqe", [20, 7])
def test_device_route_cuts_long_lists_as_the_host_route_does(built, mqe):
    """the built model's lists hold up to 20 entries: a cap at the longest list's length cuts nothing, one below it does"""
    algo, model = built
    longest = max(int(np.diff(c.row_ptr.cpu().numpy()).max()) for c in model.correlators)
    assert longest == 20
    qs = [{"item": i} for i in range(model.n_items)] + [{"item": i, "itemBias": -1, "num": 7} for i in range(0, model.n_items, 3)] + [{"item": 60}, {"item": -1}]
    saved = with_max_query_events(algo, mqe)
    try:
        want = algo.batch_predict(model, qs, {})
        got = algo.batch_predict(model, qs, {}, item_rows="device")
        uncut = algo.ap.maxQueryEvents
        algo.ap.maxQueryEvents = 100
        assert (algo.batch_predict(model, qs, {}) != want) == (mqe < longest)
        algo.ap.maxQueryEvents = uncut
    finally:
        algo.ap.indicators, algo.ap.maxQueryEvents = saved
    for q, w, g in zip(qs, want, got):
        assert g == w, (mqe, q, g, w)


def table_rows(model, table):
    count, idx, score = (t.cpu().numpy() for t in table)
    return [[{"item": model.item_name(int(idx[r, j])), "score": float(score[r, j])} for j in range(int(count[r]))] for r in range(count.size)]


def check_table(algo, model, names, item_rows="host", **kw):
    """similar_items(items=names, **kw) == batch_predict([{"item": x, ...}]) row by row; returns the table"""
    q_kw = {k2: kw[k] for k, k2 in (("num", "num"), ("item_bias", "itemBias"), ("return_self", "returnSelf")) if kw.get(k) is not None}
    want = algo.batch_predict(model, [dict(q_kw, item=x) for x in names], {}, now_ms=NOW_MS, item_rows=item_rows)
    table = algo.similar_items(model, names, now_ms=NOW_MS, **kw)
    assert all(t.device == model.sess.device for t in table) and table[1].shape == table[2].shape == (len(names), kw.get("num") or algo.ap.num or 20)
    for x, w, g in zip(names, want, table_rows(model, table)):
        assert g == w["itemScores"], (kw, x, g, w)
    return table, want


def test_similar_items_on_the_handmade_model(handmade):
    algo, model, _, items = handmade
    names = [model.item_name(i) for i in range(model.n_items)]
    for rs in (None, False, True):
        for bias in (None, 2.5, -1.0):
            _, want = check_table(algo, model, names, return_self=rs, item_bias=bias, chunk=4)
            assert any(r["itemScores"] for r in want)
    check_table(algo, model, names + ["no such item"] + names[:2], chunk=3, num=2)
    check_table(algo, model, ["no such item", names[0]], item_bias=-1.0)
    saved = with_max_query_events(algo, 1)
    try:
        check_table(algo, model, names, chunk=5, num=6)
    finally:
        algo.ap.indicators, algo.ap.maxQueryEvents = saved
    # items=None is every item; entries behind count are -1 / 0.0
    count, idx, score = algo.similar_items(model, now_ms=NOW_MS, num=200)
    full = algo.similar_items(model, names, now_ms=NOW_MS, num=200)
    assert all(torch.equal(a, b) for a, b in zip((count, idx, score), full))
    dead = torch.arange(200)[None, :] >= count[:, None]
    assert bool(dead.any()) and bool((idx[dead] == -1).all()) and bool((score[dead] == 0).all())
    with pytest.raises(ValueError):
        algo.similar_items(model, num=0)
    with pytest.raises(ValueError):
        algo.similar_items(model, torch.zeros(3, dtype=torch.int64))


def test_similar_items_in_chunks_on_a_built_model(built):
    """60 items, chunk = 7: eight full chunks and a ragged one; a subset given as a tensor; the collabFiltering model (no backfill)"""
    algo, model = built
    assert model.n_items > 7 and model.n_items % 7 != 0
    names = list(range(model.n_items))
    for rs in (False, True):
        table, want = check_table(algo, model, names, return_self=rs, chunk=7)
        assert any(s["score"] > 0 for r in want for s in r["itemScores"])
        whole = algo.similar_items(model, return_self=rs)                      # one chunk
        assert all(torch.equal(a, b) for a, b in zip(table, whole))
    sub = torch.tensor([5, 59, 0, 5, 33, -1, 60, 17, 2], dtype=torch.int32)
    got = table_rows(model, algo.similar_items(model, sub, chunk=4))
    want = algo.batch_predict(model, [{"item": int(x)} for x in sub], {})
    assert [w["itemScores"] for w in want] == got
    check_table(algo, model, names[:20], item_bias=-1.0, chunk=7, num=5)
    saved = algo.recsModel
    algo.recsModel = "collabFiltering"
    try:
        _, want = check_table(algo, model, names, chunk=7, num=30)
        assert all(s["score"] > 0 for r in want for s in r["itemScores"])
    finally:
        algo.recsModel = saved


def test_the_device_route_never_reads_the_matrices_back(built, monkeypatch):
    from universal_recommender_amd.recommend import DeviceModel
    algo, model = built
    qs = [{"item": 3}, {"item": 7, "itemBias": -1}, {"item": 999}, {"item": 5, "returnSelf": True}]
    want = algo.batch_predict(model, qs, {})
    for c in model.correlators:
        c.host = None

    def refuse(self, c, i):
        raise AssertionError("DeviceModel.indicator_row was called")

    monkeypatch.setattr(DeviceModel, "indicator_row", refuse)
    with pytest.raises(AssertionError):
        algo.batch_predict(model, qs, {})
    assert algo.batch_predict(model, qs, {}, item_rows="device") == want
    algo.similar_items(model, chunk=16)
    assert all(c.host is None for c in model.correlators)
