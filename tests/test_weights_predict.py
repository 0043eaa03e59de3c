"""Term weights at the Python level (decision D20) on the simulator session, over the handmade golden's model with item properties and dates:
batch_predict, predict, similar_items and user_recommendations under term_weights="idf" against a pure-Python restatement over the model's host
matrices -- integer sums of the weights, the f64 fold in clause order, the order (score desc, item index asc) -- exactly; the dict-history, DeviceHistory
and item_rows="device" routes against each other; None against the call without the argument; evaluate against rank_metrics of the weighted table.

The weights the restatement uses are the ones the device computed (checked to one unit against numpy's idf, as in the kernel tests), so scores compare bit
for bit.  Eligibility is not restated here -- the weights do not touch it: the eligible items of a query are those the unweighted call returns."""
import numpy as np
import pytest
import torch

import recommend_weights_ref as W
from test_recommend_rules_golden import NOW_MS, _stack

UNIT = 2.0 ** -15
CAT = {"name": "categories", "values": ["Tablets", "Phones"]}


@pytest.fixture(scope="module")
def stack(sim_session):
    algo, model, _docs, history, items, *_ = _stack(sim_session)
    assert model.fill_order is None and model.n_items <= 256 and algo.ap.termWeights is None
    return algo, model, history, items


@pytest.fixture(scope="module")
def host(stack):
    """name -> (row_ptr, col_idx, n_cols, weights read back from the device) for every matrix a should-clause can stand on"""
    _, model, _, _ = stack
    tw = model.term_weights("idf")
    assert model.term_weights() is tw, "built once"
    out = {}
    for m in list(model.correlators) + list(model.properties.values()):
        rp = m.row_ptr.cpu().numpy()[: model.n_items + 1]
        ci = m.col_idx.cpu().numpy()[: int(rp[-1])]
        w = tw[m.name].cpu().numpy()
        assert w.dtype == np.uint32 and w.size == m.n_cols
        cp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=m.n_cols))])
        want = W.idf_ref(cp, max(int(np.count_nonzero(np.diff(rp))), 1))
        assert np.abs(w.astype(np.int64) - want.astype(np.int64)).max() <= 1, m.name
        out[m.name] = (rp, ci, m.n_cols, w)
    assert any(len(set(w.tolist())) > 1 for _, _, _, w in out.values()), "some matrix has terms of different rarity"
    return out


def restated_scores(algo, model, host, history, q, weighted=True):
    """score of every item for a query of the forms used below (user, item, itemSet, eventNames, positive biases, boosted fields): D20 word for word"""
    ap = algo.ap
    events = list(algo.modelEventNames)
    max_items = {i.name: (i.maxItemsPerUser if i.maxItemsPerUser is not None else 500) for i in ap.indicators} if ap.indicators else {e: 100 for e in events}
    mqe = sum(i.maxItemsPerUser if i.maxItemsPerUser is not None else 100 for i in ap.indicators) * 10 if ap.indicators else (ap.maxQueryEvents or 100)
    boost = lambda b: float(b) if b > 0 and b != 1 else 1.0
    clauses = []          # (matrix name, boost, set of columns)
    user, item = q.get("user"), q.get("item")
    for ev in [c.name for c in model.correlators]:
        if user is None or ev not in (q.get("eventNames") or events):
            continue
        c = model.by_name[ev]
        recent = list(reversed(history.get(user, {}).get(ev, [])))[: max_items.get(ev, 100)]
        cols = {model.column_index(c, i) for i in recent} - {None}
        clauses.append((ev, boost(q.get("userBias", 1.0)), cols))
    i = model.item_index(item) if item is not None else None
    if i is not None:
        for ev in events:
            rp, ci, _, _ = host[ev]
            ids = ci[rp[i]:rp[i + 1]]
            if ids.size > mqe:
                ids = ids[: mqe - 1]
            clauses.append((ev, boost(q.get("itemBias", 1.0)), set(ids.tolist())))
    for f in q.get("fields") or []:
        assert f["bias"] > 0, "the restatement covers boosts only"
        prop = model.properties[f["name"]]
        clauses.append((f["name"], float(f["bias"]), {prop.values[v] for v in f["values"] if v in prop.values}))
    if q.get("itemSet"):
        c = model.by_name[events[0]]
        clauses.append((events[0], 1.0, {model.column_index(c, x) for x in q["itemSet"]} - {None}))
    scores = []
    for it in range(model.n_items):
        s = 0.0
        for name, b, cols in clauses:
            rp, ci, _, w = host[name]
            shared = cols & set(ci[rp[it]:rp[it + 1]].tolist())
            m = sum(int(w[h]) if weighted else W.ONE for h in shared)          # a Python int: exact
            s = s + b * (float(m) * UNIT)
        scores.append(s)
    return scores


def restated_answer(algo, model, host, history, q, eligible, weighted=True):
    scores = restated_scores(algo, model, host, history, q, weighted)
    order = sorted((model.item_index(x) for x in eligible), key=lambda it: (-scores[it], it))
    return [{"item": model.item_name(it), "score": scores[it]} for it in order]


def scored_queries(history, items):
    users = list(history)
    qs = [{"user": u} for u in users] + [{"item": i} for i in items] + [{"user": u, "item": items[k % len(items)]} for k, u in enumerate(users)]
    qs += [{"user": users[0], "eventNames": ["view"]}, {"user": users[1], "userBias": 2.5, "item": items[0], "itemBias": 0.5}, {"itemSet": items[1:4]},
           {"user": users[2], "itemSet": items[:2]}, {"item": items[2], "returnSelf": True}]
    qs += [{"user": u, "fields": [dict(CAT, bias=2.5)]} for u in users[:3]] + [{"item": items[1], "fields": [dict(CAT, bias=20), {"name": "countries", "values": ["United States"], "bias": 3}]}]
    return qs


def other_queries(history, items):
    """filters, negative biases, paging, unknown ids: compared between the routes, not restated"""
    users = list(history)
    return [{}, {"user": "nobody"}, {"item": "no such item"}, {"user": users[0], "fields": [dict(CAT, bias=-1)]}, {"user": users[1], "fields": [dict(CAT, bias=0)]},
            {"user": users[0], "userBias": -1}, {"item": items[0], "itemBias": -1}, {"user": users[1], "item": items[1], "itemBias": -1, "userBias": -1},
            {"item": items[2], "from": 1, "num": 3}, {"user": users[2], "num": 2}, {"item": items[0], "blacklistItems": items[1:3]}]


def full(model, qs):
    return [dict(q, num=model.n_items) for q in qs]


def test_batch_predict_and_predict_equal_the_restatement(stack, host):
    algo, model, history, items = stack
    qs = full(model, scored_queries(history, items))
    plain = algo.batch_predict(model, qs, history, now_ms=NOW_MS)
    got = algo.batch_predict(model, qs, history, now_ms=NOW_MS, term_weights="idf")
    differs = 0
    for q, p, g in zip(qs, plain, got):
        eligible = [s["item"] for s in p["itemScores"]]
        assert p["itemScores"] == restated_answer(algo, model, host, history, q, eligible, weighted=False), q      # the restatement restates D15 too
        assert g["itemScores"] == restated_answer(algo, model, host, history, q, eligible), q                       # items AND score bits
        differs += g != p
    assert differs > len(qs) // 2 and any(s["score"] > 0 for g in got for s in g["itemScores"])
    for q, g in list(zip(qs, got))[::5]:
        assert algo.predict(model, q, history, now_ms=NOW_MS, term_weights="idf") == g


def test_a_boosted_fields_clause_is_weighted(stack, host):
    algo, model, history, items = stack
    user = list(history)[0]
    q = {"user": user, "num": model.n_items}
    qf = dict(q, fields=[dict(CAT, bias=2.5)])
    base = {s["item"]: s["score"] for s in algo.predict(model, q, history, now_ms=NOW_MS, term_weights="idf")["itemScores"]}
    boosted = {s["item"]: s["score"] for s in algo.predict(model, qf, history, now_ms=NOW_MS, term_weights="idf")["itemScores"]}
    rp, ci, _, w = host["categories"]
    prop = model.properties["categories"]
    cols = {prop.values[v] for v in CAT["values"]}
    assert any(int(w[h]) != W.ONE for h in cols), "the property's values do not weigh 1.0"
    raised = 0
    for name, s in boosted.items():
        it = model.item_index(name)
        m = sum(int(w[h]) for h in cols & set(ci[rp[it]:rp[it + 1]].tolist()))
        assert s == base[name] + 2.5 * (float(m) * UNIT), name
        raised += m > 0
    assert raised >= 1


def test_some_top_num_order_differs_from_the_unweighted_one(stack, host):
    algo, model, history, items = stack
    num = 3
    qs = scored_queries(history, items)
    plain = algo.batch_predict(model, full(model, qs), history, now_ms=NOW_MS)
    picked = []
    for q, p in zip(qs, plain):
        eligible = [s["item"] for s in p["itemScores"]]
        a = [s["item"] for s in restated_answer(algo, model, host, history, q, eligible, weighted=False)[:num]]
        b = [s["item"] for s in restated_answer(algo, model, host, history, q, eligible)[:num]]
        if a != b:
            picked.append((q, a, b))
    assert picked, "the restatement finds a query whose top 3 changes under idf"
    for q, a, b in picked:
        q = dict(q, num=num)
        assert [s["item"] for s in algo.predict(model, q, history, now_ms=NOW_MS)["itemScores"]] == a
        assert [s["item"] for s in algo.predict(model, q, history, now_ms=NOW_MS, term_weights="idf")["itemScores"]] == b


def test_the_routes_agree_bit_for_bit(sim_session, stack):
    from universal_recommender_amd.history import DeviceHistory
    algo, model, history, items = stack
    dh = DeviceHistory.from_dict(sim_session, model, history)
    qs = scored_queries(history, items) + other_queries(history, items)
    want = algo.batch_predict(model, qs, history, now_ms=NOW_MS, term_weights="idf")
    for hist, rows in ((dh, "host"), (history, "device"), (dh, "device")):
        got = algo.batch_predict(model, qs, hist, now_ms=NOW_MS, item_rows=rows, term_weights="idf")
        for q, w, g in zip(qs, want, got):
            assert g == w, (rows, type(hist).__name__, q, g, w)
    # the dict of the model's own arrays is "idf"; an empty dict and names the model does not know weigh every term 1.0
    assert algo.batch_predict(model, qs, history, now_ms=NOW_MS, term_weights=dict(model.term_weights("idf"))) == want
    plain = algo.batch_predict(model, qs, history, now_ms=NOW_MS)
    assert algo.batch_predict(model, qs, history, now_ms=NOW_MS, term_weights={}) == plain
    assert algo.batch_predict(model, qs, history, now_ms=NOW_MS, term_weights={"no such event": torch.ones(3, dtype=torch.uint32)}) == plain
    assert plain != want


def test_none_is_the_call_without_the_argument_and_the_parameter_is_the_default(sim_session, stack):
    from universal_recommender_amd.history import DeviceHistory
    from universal_recommender_amd.ur_algorithm import URAlgorithmParams
    algo, model, history, items = stack
    dh = DeviceHistory.from_dict(sim_session, model, history)
    qs = scored_queries(history, items) + other_queries(history, items)
    plain = algo.batch_predict(model, qs, history, now_ms=NOW_MS)
    weighted = algo.batch_predict(model, qs, history, now_ms=NOW_MS, term_weights="idf")
    assert algo.batch_predict(model, qs, history, now_ms=NOW_MS, term_weights=None) == plain
    assert algo.predict(model, qs[0], history, now_ms=NOW_MS, term_weights=None) == algo.predict(model, qs[0], history, now_ms=NOW_MS) == plain[0]
    for a, b in ((algo.similar_items(model, now_ms=NOW_MS, term_weights=None), algo.similar_items(model, now_ms=NOW_MS)),
                 (algo.user_recommendations(model, dh, now_ms=NOW_MS, term_weights=None), algo.user_recommendations(model, dh, now_ms=NOW_MS))):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert URAlgorithmParams.from_engine_json({"algorithms": [{"name": "ur", "params": {"termWeights": "idf"}}]}).termWeights == "idf"
    algo.ap.termWeights = "idf"
    try:
        assert algo.batch_predict(model, qs, history, now_ms=NOW_MS) == weighted
        assert algo.batch_predict(model, qs, history, now_ms=NOW_MS, term_weights="none") == plain
        assert all(torch.equal(x, y) for x, y in zip(algo.similar_items(model, now_ms=NOW_MS), algo.similar_items(model, now_ms=NOW_MS, term_weights="idf")))
    finally:
        algo.ap.termWeights = None
    for bad in ("bm25", 3, {"purchase": torch.ones(model.by_name["purchase"].n_cols, dtype=torch.int32)}, {"purchase": torch.ones(1, dtype=torch.uint32)}):
        with pytest.raises(ValueError):
            algo.batch_predict(model, qs[:1], history, now_ms=NOW_MS, term_weights=bad)


def table_rows(model, table):
    count, idx, score = (t.cpu().numpy() for t in table)
    return [[{"item": model.item_name(int(idx[r, j])), "score": float(score[r, j])} for j in range(int(count[r]))] for r in range(count.size)]


def test_similar_items_equals_the_restatement(stack, host):
    algo, model, history, items = stack
    names = [model.item_name(i) for i in range(model.n_items)]
    num = model.n_items
    plain = table_rows(model, algo.similar_items(model, names, num=num, now_ms=NOW_MS))
    for chunk in (4, 65536):
        table = algo.similar_items(model, names, num=num, now_ms=NOW_MS, chunk=chunk, term_weights="idf")
        assert all(t.device == model.sess.device for t in table)
        for x, p, g in zip(names, plain, table_rows(model, table)):
            assert g == restated_answer(algo, model, host, history, {"item": x}, [s["item"] for s in p]), x
    got = table_rows(model, algo.similar_items(model, names + ["no such item"], num=5, item_bias=2.5, return_self=True, now_ms=NOW_MS, term_weights="idf"))
    want = algo.batch_predict(model, [{"item": x, "num": 5, "itemBias": 2.5, "returnSelf": True} for x in names + ["no such item"]], {}, now_ms=NOW_MS, term_weights="idf")
    assert got == [w["itemScores"] for w in want]
    # as a filter the lists carry no weight
    a, b = algo.similar_items(model, names, item_bias=-1.0, now_ms=NOW_MS, term_weights="idf"), algo.similar_items(model, names, item_bias=-1.0, now_ms=NOW_MS)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_user_recommendations_equals_the_restatement(sim_session, stack, host):
    from universal_recommender_amd.history import DeviceHistory
    algo, model, history, items = stack
    dh = DeviceHistory.from_dict(sim_session, model, history)
    users = list(history)
    num = model.n_items
    plain = table_rows(model, algo.user_recommendations(model, dh, users, num=num, now_ms=NOW_MS))
    for chunk in (3, 65536):
        table = algo.user_recommendations(model, dh, users, num=num, now_ms=NOW_MS, chunk=chunk, term_weights="idf")
        for u, p, g in zip(users, plain, table_rows(model, table)):
            assert g == restated_answer(algo, model, host, history, {"user": u}, [s["item"] for s in p]), u
    assert plain != table_rows(model, table)
    got = table_rows(model, algo.user_recommendations(model, dh, users + ["nobody"], num=4, event_names=["view"], user_bias=2.5, now_ms=NOW_MS, term_weights="idf"))
    want = algo.batch_predict(model, [{"user": u, "num": 4, "eventNames": ["view"], "userBias": 2.5} for u in users + ["nobody"]], dh, now_ms=NOW_MS, term_weights="idf")
    assert got == [w["itemScores"] for w in want]
    a, b = algo.user_recommendations(model, dh, user_bias=-1.0, now_ms=NOW_MS, term_weights="idf"), algo.user_recommendations(model, dh, user_bias=-1.0, now_ms=NOW_MS)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_evaluate_equals_rank_metrics_of_the_weighted_table(sim_session, stack):
    from universal_recommender_amd.evaluate import log2_discount
    from universal_recommender_amd.history import DeviceHistory
    from universal_recommender_amd.recommend import _csr
    algo, model, history, items = stack
    sess = sim_session
    train = DeviceHistory.from_dict(sess, model, history)
    in_model = [model.item_name(i) for i in range(model.n_items)]
    held_out = {u: {"purchase": [in_model[(k + j) % len(in_model)] for j in range(k % 3)]} for k, u in enumerate(history)}     # every third user has no truth item
    test = DeviceHistory.from_dict(sess, model, held_out)
    ks, num = (1, 3, 5), 6
    got = algo.evaluate(model, train, test, ks=ks, num=num, now_ms=NOW_MS, term_weights="idf")
    count, idx, _ = algo.user_recommendations(model, train, num=num, now_ms=NOW_MS, term_weights="idf")
    truth = _csr([np.unique(np.array([model.item_index(x) for x in held_out[u]["purchase"]], np.int64)) for u in history], sess.device)
    hits, ap, ndcg, s_i, _ = sess.rank_metrics(count, idx, truth[0], truth[1], ks, torch.from_numpy(log2_discount(num)).to(sess.device))
    tree_ap, tree_ndcg = sess.tree_sum(ap), sess.tree_sum(ndcg)
    sess.synchronize()
    evaluated = int(s_i[0])
    assert evaluated == sum(1 for k in range(len(history)) if k % 3) == got["evaluated"] and got["not_evaluated"] == len(history) - evaluated
    assert torch.equal(got["per_user"]["hits"], hits) and torch.equal(got["per_user"]["ap"], ap) and torch.equal(got["per_user"]["ndcg"], ndcg)
    assert got["map"] == [float(v) / evaluated for v in tree_ap.tolist()] and got["ndcg"] == [float(v) / evaluated for v in tree_ndcg.tolist()]
    assert got["precision"] == [int(s_i[2 + x]) / (evaluated * k) for x, k in enumerate(ks)]
    # None is the evaluation without the argument; a list of event mixes passes the weights on
    a, b = algo.evaluate(model, train, test, ks=ks, num=num, now_ms=NOW_MS, term_weights=None), algo.evaluate(model, train, test, ks=ks, num=num, now_ms=NOW_MS)
    assert {k: v for k, v in a.items() if k != "per_user"} == {k: v for k, v in b.items() if k != "per_user"} and torch.equal(a["per_user"]["ap"], b["per_user"]["ap"])
    two = algo.evaluate(model, train, test, ks=ks, num=num, event_names=[["purchase"], ["view"]], now_ms=NOW_MS, term_weights="idf")
    for mix, rep in zip((["purchase"], ["view"]), two):
        c2, i2, _ = algo.user_recommendations(model, train, num=num, event_names=mix, now_ms=NOW_MS, term_weights="idf")
        h2 = sess.rank_metrics(c2, i2, truth[0], truth[1], ks, torch.from_numpy(log2_discount(num)).to(sess.device))[0]
        assert torch.equal(rep["per_user"]["hits"], h2)
