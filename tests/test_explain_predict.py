"""batch_predict(explain=E) / user_recommendations(explain=E) on the host simulator over the handmade golden data (the stack of
tests/test_recommend_rules_golden.py): every item score's "because" list against a restatement from the host model and the dict history -- per clause the
intersection of the query's terms with the result item's own row, sorted by (-boost, clause, column) and cut to E."""
import pytest

from test_recommend_rules_golden import NOW_MS, _stack

QUERIES = [{"user": "u1"}, {"user": "U 2", "num": 3, "from": 1}, {"item": "Iphone 4"}, {"itemSet": ["Iphone 6", "Nexus"]},
           {"user": "u1", "fields": [{"name": "categories", "values": ["Tablets", "Phones"], "bias": 2.5}]}, {"user": "nobody"}]


@pytest.fixture(scope="module")
def stack(sim_session):
    from universal_recommender_amd.history import DeviceHistory
    algo, model, _, history, *_ = _stack(sim_session)
    return algo, model, history, DeviceHistory.from_dict(sim_session, model, history)


def because(model, history, q, item, e):
    """the clauses in batch_predict's order: user history per event, the query item's lists per event, boosted fields, the item set"""
    i, found, first = model.item_index(item), [], model.correlators[0]
    cols = lambda c, ids: {model.column_index(c, x) for x in ids} - {None}
    plan = [("user", c.name, c, 1.0, cols(c, history.get(q.get("user"), {}).get(c.name, []))) for c in model.correlators]
    plan += [("item", c.name, c, 1.0, set(model.indicator_row(c, model.item_index(q["item"])).tolist())) for c in model.correlators if "item" in q]
    plan += [("field", f["name"], model.properties[f["name"]], f["bias"], {model.properties[f["name"]].values[v] for v in f["values"]}) for f in q.get("fields", [])]
    plan += [("itemSet", first.name, first, 1.0, cols(first, q.get("itemSet", [])))]
    for clause, (_, _, mat, boost, terms) in enumerate(plan):
        rp, ci = mat.row_ptr.cpu().numpy(), mat.col_idx.cpu().numpy()
        found += [(-boost, clause, h) for h in set(ci[rp[i]:rp[i + 1]].tolist()) & terms]
    name = lambda mat, h: {v: k for k, v in mat.values.items()}[h] if hasattr(mat, "values") else mat.column_ids.inverse(h)
    return [{"clause": plan[c][0], "name": plan[c][1], "term": name(plan[c][2], h), "weight": -b} for b, c, h in sorted(found)[:e]]


@pytest.mark.parametrize("device_history", [False, True])
def test_because_lists(stack, device_history):
    algo, model, history, dh = stack
    hist = dh if device_history else history
    plain = algo.batch_predict(model, QUERIES, hist, now_ms=NOW_MS)
    got = algo.batch_predict(model, QUERIES, hist, now_ms=NOW_MS, explain=3)
    assert plain == algo.batch_predict(model, QUERIES, hist, now_ms=NOW_MS, explain=None) and algo.predict(model, QUERIES[0], hist, now_ms=NOW_MS, explain=3) == got[0]
    for q, p, g in zip(QUERIES, plain, got):
        assert [{k: v for k, v in s.items() if k != "because"} for s in g["itemScores"]] == p["itemScores"], q
        for s in g["itemScores"]:
            assert s["because"] == because(model, history, q, s["item"], 3) and (s["because"] == []) == (s["score"] == 0.0), (q, s)
    assert {"user", "item", "itemSet", "field"} == {b["clause"] for g in got for s in g["itemScores"] for b in s["because"]}
    with pytest.raises(ValueError):
        algo.batch_predict(model, QUERIES, hist, explain=65)


def test_user_recommendations_rows_are_batch_predict_s(stack):
    algo, model, history, dh = stack
    users = list(history) + ["nobody"]
    want = algo.batch_predict(model, [{"user": u, "num": 6} for u in users], dh, now_ms=NOW_MS, explain=3)
    assert len(algo.user_recommendations(model, dh, users, num=6, now_ms=NOW_MS)) == 3
    count, idx, score, n, clause, term, contrib, names = algo.user_recommendations(model, dh, users, num=6, chunk=2, now_ms=NOW_MS, explain=3)
    for r, w in enumerate(want):
        why = lambda j, x: dict(zip(("clause", "name"), names[int(clause[r, j, x])]), weight=float(contrib[r, j, x]),
                                term=model.by_name[names[int(clause[r, j, x])][1]].column_ids.inverse(int(term[r, j, x])))
        rows = [{"item": model.item_name(int(idx[r, j])), "score": float(score[r, j]), "because": [why(j, x) for x in range(int(n[r, j]))]} for j in range(int(count[r]))]
        assert rows == w["itemScores"] and not n[r, int(count[r]):].any(), users[r]
    assert int(n.sum()) > 0
