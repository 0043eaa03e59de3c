"""Item properties from the device-resident property store (decision D25 of DESIGN.md) through the whole stack, on the simulator session the other
predict tests use, with the reference's integration golden (tests/golden/handmade.json, tests/test_recommend_rules_golden.py's stack).

A model whose properties come from DeviceProperties.from_property_map + DeviceModel.set_properties holds the tensors of
DeviceModel.from_indicators(properties=...) and answers all 28 golden queries identically.  Then a $set moves one item out of `Tablets`, an $unset removes
another item's `countries` and a $delete removes a third item: the answers are those of a model rebuilt on the host from the aggregated map of
tests/props_ref.py with the reference's deleted mask as item_mask, and differ from the answers before the events."""
import json

import numpy as np
import pytest
import torch

import props_ref as P
from test_recommend_rules_golden import DAY_MS, NOW_MS, _iso, _render, _stack


def _property_map(doc, dates, props):
    """the aggregated map test_recommend_rules_golden._stack builds its model from"""
    properties = {item: dict(p) for item, p in props.items()}
    for item, d in dates.items():
        properties.setdefault(item, {}).update({"date": _iso(NOW_MS + round(d["date"] * DAY_MS)), "available": _iso(NOW_MS + round(d["available"] * DAY_MS)),
                                                "expires": _iso(NOW_MS + round(d["expires"] * DAY_MS))})
    return properties


def _bare(model):
    """the same indicators and dictionaries, no properties"""
    from universal_recommender_amd.recommend import DeviceModel
    return DeviceModel(model.sess, model.item_ids, model.n_items, model.correlators, model.fill_order)


def _by_column(col_ptr, row_idx, n_rows):
    """the entries of a CSC as sorted (column, row) keys"""
    cp = col_ptr.cpu().long()
    col = torch.repeat_interleave(torch.arange(cp.numel() - 1), cp[1:] - cp[:-1])
    return torch.sort(col * n_rows + row_idx.cpu().long()[: col.numel()]).values


def _split(events, index_of):
    """Generic property events -> per property the stream ((item id, time, kind) and the value per position) and the delete stream: the splitting
    DeviceProperties.apply documents, restated"""
    streams, deletes = {}, []
    for item, kind, props, t in events:
        i = index_of(item)
        if i is None:
            continue
        if kind == "$delete":
            deletes.append((i, t))
        elif kind == "$unset":
            for name in props:
                ev, vals = streams.setdefault(name, ([], []))
                ev.append((i, t, P.UNSET))
                vals.append(None)
        else:
            for name, value in props.items():
                ev, vals = streams.setdefault(name, ([], []))
                ev.append((i, t, P.SET))
                vals.append(value)
    return streams, deletes


def _answers(algo, model, queries, history, mask=None, **kw):
    return algo.batch_predict(model, queries, history, mask, now_ms=NOW_MS, **kw)


def _flow(sess):
    from universal_recommender_amd.properties import DeviceProperties
    from universal_recommender_amd.recommend import _device_properties
    algo, model, docs, history, items, doc, dates, props = _stack(sess)
    properties = _property_map(doc, dates, props)
    queries = [_render(q["query"]) for q in doc["queries"]]
    wide = [{k: v for k, v in q.items() if k not in ("num", "from")} | {"num": model.n_items} for q in queries]
    assert len(queries) == 28

    # 1. from_property_map + set_properties == from_indicators(properties=...): CSR, CSC, dates, and every golden answer
    dp = DeviceProperties.from_property_map(sess, model, properties, algo.dateNames)
    m2 = _bare(model)
    assert m2.set_properties(dp) is m2
    assert list(m2.properties) == list(model.properties) and list(m2.dates) == list(model.dates) == algo.dateNames
    for name, a in model.properties.items():
        b = m2.properties[name]
        assert (b.name, b.n_cols, b.values) == (a.name, a.n_cols, a.values), name
        for f in ("row_ptr", "col_idx", "col_ptr", "row_idx"):
            x, y = getattr(a, f), getattr(b, f)
            assert x.dtype == y.dtype and x.shape == y.shape, (name, f)
            if f == "row_idx":      # urcco_dev_transpose leaves the order inside a column unspecified: equal column by column, as sets
                x, y = _by_column(a.col_ptr, x, model.n_items), _by_column(b.col_ptr, y, model.n_items)
            assert torch.equal(x, y), (name, f, x, y)
    for name, a in model.dates.items():
        assert a.dtype == m2.dates[name].dtype and torch.equal(a, m2.dates[name]), name
    assert int(dp.item_mask().min()) == 1
    before, before_wide = _answers(algo, model, queries, history), _answers(algo, model, wide, history)
    assert _answers(algo, m2, queries, history) == before and _answers(algo, m2, wide, history) == before_wide
    idf_before = {k: v.clone() for k, v in m2.term_weights("idf").items()}

    # 2. an inventory change: Nexus leaves Tablets, Iphone 4 loses its countries, Galaxy is deleted, Ipad-retina expires later
    in_model = [model.item_name(i) for i in range(model.n_items)]
    assert {"Nexus", "Iphone 4", "Galaxy", "Ipad-retina"} <= set(in_model)
    events = [("Nexus", "$set", {"categories": ["Phones", "Electronics", "Google", "Refurbished"]}, 10), ("Iphone 4", "$unset", ["countries"], 10), ("Galaxy", "$delete", None, 10),
              ("Ipad-retina", "$set", {"expires": _iso(NOW_MS + 30 * DAY_MS)}, 11), ("Surface", "$set", {"categories": ["Phones"]}, 12), ("Nexus", "$set", {"weight": 3}, 12)]
    assert dp.apply(events) is dp
    m2.set_properties(dp)
    mask = dp.item_mask()
    # the reference: the rule over ALL events, then the host path over its aggregated map
    loaded = [(item, "$set", fields, 0) for item, fields in properties.items()]
    streams, deletes = _split(loaded + events, model.item_index)
    D = P.aggregate_deletes(model.n_items, deletes)
    agg = {name: P.aggregate(model.n_items, ev) + (vals,) for name, (ev, vals) in streams.items()}
    served = {name: v for name, v in agg.items() if name in algo.dateNames or all(isinstance(x, list) for x in v[2] if x is not None)}
    assert set(agg) - set(served) == {"weight"}                                # neither a list of strings nor a date: ignored
    host_map = P.aggregated_map(model.n_items, model.item_name, served, D)
    assert "Tablets" not in host_map["Nexus"]["categories"] and "countries" not in host_map["Iphone 4"] and "Galaxy" not in host_map
    w_mask = P.exists_mask(model.n_items, [S for S, _, _ in served.values()], D)
    assert np.array_equal(mask.cpu().numpy(), w_mask) and w_mask.sum() == model.n_items - 1 and w_mask[model.item_index("Galaxy")] == 0
    m3 = _bare(model)
    m3.properties, m3.dates = _device_properties(sess, host_map, algo.dateNames, model.n_items, model.item_index)
    for name, a in m3.properties.items():                                       # the same matrices up to the order of the value dictionary
        b = m2.properties[name]
        rows = lambda m: [sorted(k for k, c in m.values.items() if c in set(m.col_idx[int(m.row_ptr[i]):int(m.row_ptr[i + 1])].tolist())) for i in range(model.n_items)]  # noqa: E731
        assert rows(a) == rows(b), name
    for name, a in m3.dates.items():
        assert torch.equal(a, m2.dates[name]), name
    after, after_wide = _answers(algo, m2, queries, history, mask), _answers(algo, m2, wide, history, mask)
    assert after == _answers(algo, m3, queries, history, w_mask) and after_wide == _answers(algo, m3, wide, history, w_mask)
    assert after != before and after_wide != before_wide
    tablets = _answers(algo, m2, [{"fields": [{"name": "categories", "values": ["Tablets"], "bias": -1}], "num": 7}], history, mask)[0]["itemScores"]
    assert [s["item"] for s in tablets] == ["Ipad-retina"]
    assert all(s["item"] != "Galaxy" for res in after_wide for s in res["itemScores"])
    assert any(s["item"] == "Galaxy" for res in before_wide for s in res["itemScores"])

    # 3. term_weights="idf" after set_properties is computed from the new matrices
    idf = m2.term_weights("idf")
    for name, p in m2.properties.items():
        rp = p.row_ptr[: model.n_items + 1]
        n_docs = max(int((rp[1:] > rp[:-1]).sum()), 1)
        assert torch.equal(idf[name], sess.idf_weights(p.col_ptr, p.n_cols, n_docs)), name
    assert idf["categories"].numel() != idf_before["categories"].numel() or not torch.equal(idf["categories"], idf_before["categories"])
    boosted = [q for q in wide if any(f.get("bias", 0) > 0 for f in q.get("fields", []))]
    assert len(boosted) >= 4
    assert _answers(algo, m2, boosted, history, mask, term_weights="idf") == _answers(algo, m3, boosted, history, w_mask, term_weights="idf")

    # properties_from_events: the one-line form
    dp2 = algo.properties_from_events(_bare(model), loaded + events)
    m4 = _bare(model).set_properties(dp2)
    assert torch.equal(dp2.item_mask(), mask) and _answers(algo, m4, queries, history, mask) == after
    with pytest.raises(ValueError):
        dp.apply([("Nexus", "$merge", {}, 1)])
    # a grown catalogue: the zero-extended state knows nothing about the new items and keeps everything about the old ones
    n = model.n_items
    assert dp2.grow(n + 5) is dp2 and dp2.item_mask().cpu().tolist() == w_mask.tolist() + [1] * 5
    grown, grown_dates = dp2.materialise()
    for name, p in m4.properties.items():
        assert torch.equal(grown[name].row_ptr[: n + 1], p.row_ptr) and torch.equal(grown[name].col_idx, p.col_idx) and int(grown[name].row_ptr[-1]) == int(p.row_ptr[-1])
    assert all(torch.equal(grown_dates[k][:n], m4.dates[k]) and (grown_dates[k][n:] == P.I64_MIN).all() for k in m4.dates)
    with pytest.raises(ValueError):
        dp2.grow(n)
    with pytest.raises(ValueError):
        _bare(model).set_properties(dp2)
    json.dumps(after)     # plain Python all the way


def test_properties_from_the_device_store_on_the_simulator(sim_session):
    _flow(sim_session)


@pytest.mark.gpu
def test_properties_from_the_device_store_on_the_gpu(gpu_session):
    _flow(gpu_session)
