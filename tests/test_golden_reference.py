"""Pins the oracle (and, through the simulator build, the host mirror + C ABI orchestration) against the ONLY golden
vectors the reference holds for the CCO path: the two integration-test expected files (committed here as JSON by
tests/golden/make_golden.py).  They pin indicator MEMBERSHIP -- which ids sit in which item's indicator fields -- and
through it the Preparator user filter (minEventsPerUser on raw counts), N = size of the user dictionary, the duplicate
collapse, the drop of secondary-event users absent from the primary, and the zero-LLR drop.  LLR magnitudes, list
order and the top-k cut never reach a golden (package.scala:102-104 discards scores): see oracle/cco_oracle.py."""
import json
import os

import pytest

from membership import handmade_dates, item_properties, positive_items
from oracle import cco_oracle as PO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    doc = json.load(open(os.path.join(GOLDEN, name)))
    by_event, history, items = {}, {}, []
    for u, e, i in doc["events"]:
        by_event.setdefault(e, []).append((u, i))
        history.setdefault(u, {}).setdefault(e, []).append(i)
        if i not in items:
            items.append(i)
    return doc, by_event, history, items


def _oracle_model(doc, by_event, min_events_override="from-json"):
    names = doc["datasource_params"]["eventNames"]
    min_events = doc["datasource_params"].get("minEventsPerUser") if min_events_override == "from-json" else min_events_override
    prepared = PO.prepare(PO.split_actions(by_event, names), min_events)
    ap = dict(doc["algorithm_params"])
    ap["seed"] = 1
    model = {}
    for name, ind in PO.calc_all(prepared, ap):
        for item, m in PO.to_string_map(name, ind).items():
            model.setdefault(item, {}).update(m)
    return model, prepared


def _check_queries(doc, model, history, items, props, primary, dates):
    """Number of golden queries whose positive-score item set the model reproduces."""
    ok = 0
    mismatches = []
    for q in doc["queries"]:
        num = q["query"].get("num", doc["algorithm_params"].get("num", 20))
        start = q["query"].get("from", 0)
        expected_pos = [s["item"] for s in q["itemScores"] if s["score"] > 0]
        expected_all = [s["item"] for s in q["itemScores"]]
        cands, pos = positive_items(q["query"], model, items, history, props, primary, dates)
        good = set(expected_all) <= set(cands)                      # nothing filtered / blacklisted shows up
        if len(pos) <= start:
            good &= expected_pos == []
        elif len(pos) - start <= num:
            good &= set(expected_pos) == set(pos) if start == 0 else set(expected_pos) <= set(pos)
        else:
            good &= len(expected_pos) == num and set(expected_pos) <= set(pos)
        ok += good
        if not good:
            mismatches.append((q["title"], q["query"], expected_pos, pos))
    return ok, mismatches


def test_handmade_golden_28_queries_pin_the_oracle():
    doc, by_event, history, items = _load("handmade.json")
    assert doc["datasource_params"]["minEventsPerUser"] == 3
    model, prepared = _oracle_model(doc, by_event)
    assert [(d.nrow, d.ncol, sum(len(r) for r in d.rows)) for _, d in prepared] == [(3, 6, 11), (3, 4, 10), (3, 2, 5)]
    props = item_properties(doc["sets"])
    ok, mism = _check_queries(doc, model, history, items, props, "purchase", handmade_dates())
    assert ok == 28, mism
    # items with no indicators at all (golden line 50 "item: Galaxy" -> all 0.0)
    assert "Galaxy" not in model and "Iphone 5" not in model
    # negative control: without the Preparator's user filter the goldens are NOT reproduced -> they do pin D1
    model_nofilter, _ = _oracle_model(doc, by_event, min_events_override=None)
    ok_nf, _ = _check_queries(doc, model_nofilter, history, items, props, "purchase", handmade_dates())
    assert ok_nf < 28


def test_item_set_golden_7_queries_pin_the_oracle():
    doc, by_event, history, items = _load("item_sets.json")
    model, prepared = _oracle_model(doc, by_event)
    ok, mism = _check_queries(doc, model, history, items, {}, "purchase", None)
    assert ok == 7, mism


def test_derived_indicator_lists_and_known_answers():
    """The indicator lists SURVEY 8c derives from the handmade data (raw LLR) + LogLikelihood known answers."""
    doc, by_event, _, _ = _load("handmade.json")
    _, prepared = _oracle_model(doc, by_event)
    res = dict(PO.calc_all(prepared, {**doc["algorithm_params"], "seed": 1}))

    def rows(name):
        ind = res[name]
        return {ind.row_ids.inverse(i): [(ind.column_ids.inverse(j), round(s, 6)) for j, s in r] for i, r in enumerate(ind.rows) if r}

    assert rows("purchase") == {"Iphone 6": [("Ipad-retina", 3.819085), ("Iphone 4", 1.046496)],
                                "Iphone 4": [("Iphone 6", 1.046496), ("Ipad-retina", 1.046496)],
                                "Ipad-retina": [("Iphone 6", 3.819085), ("Iphone 4", 1.046496)]}
    assert rows("view") == {"Iphone 6": [("Soap", 1.046496)], "Iphone 4": [("Soap", 3.819085), ("Tablets", 1.046496)],
                            "Ipad-retina": [("Soap", 1.046496)], "Nexus": [("Tablets", 1.046496)]}
    assert set(rows("category-pref")) == {"Iphone 6", "Iphone 4", "Ipad-retina", "Nexus"}
    assert [res[n].pairs for n in ("purchase", "view", "category-pref")] == [43, 36, 19]
    assert PO.log_likelihood_ratio(1, 1, 0, 2) == pytest.approx(1.7260924347106847, abs=1e-15)
    assert PO.log_likelihood_ratio(1, 1, 1, 1) == 0.0


def test_host_mirror_builds_the_same_model_as_the_oracle(sim_lib):
    """DataSource -> Preparator -> URAlgorithm.calcAll -> toStringMap of the package (C ABI host level; kernels on the
    test-only simulator here, on the GPU in tests/test_gpu_parity.py) gives the oracle's model documents."""
    from universal_recommender_amd.data_source import DataSource, DataSourceParams
    from universal_recommender_amd.preparator import Preparator
    from universal_recommender_amd.ur_algorithm import URAlgorithm, URAlgorithmParams, toStringMap
    for name in ("handmade.json", "item_sets.json"):
        doc, by_event, _, _ = _load(name)
        lines = [",".join(e) for e in doc["events"]] + [f"{i},$set,{p}" for i, p in doc["sets"]]
        engine = {"datasource": {"params": doc["datasource_params"]}, "algorithms": [{"name": "ur", "params": doc["algorithm_params"]}]}
        td = DataSource(DataSourceParams.from_engine_json(engine)).readTraining(lines)
        pd = Preparator().prepare(td)
        ap = URAlgorithmParams.from_engine_json(engine)
        ap.seed = 1
        model = {}
        for ev, ind in URAlgorithm(ap, library=sim_lib).train(pd).coocurrenceMatrices:
            for item, m in toStringMap(ind, ev).items():
                model.setdefault(item, {}).update(m)
        ref, _ = _oracle_model(doc, by_event)
        assert model == ref


def test_model_documents_match_the_oracle_and_the_reference_document_shape(sim_lib, tmp_path):
    """URModel.save's per-item documents (URModel.scala:57-75): {id, <event>: [ids strongest first], ...props}."""
    from universal_recommender_amd.data_source import DataSource, DataSourceParams
    from universal_recommender_amd.preparator import Preparator
    from universal_recommender_amd.ur_algorithm import URAlgorithm, URAlgorithmParams
    from universal_recommender_amd.ur_model import URModel
    doc, by_event, _, items = _load("handmade.json")
    lines = [",".join(e) for e in doc["events"]] + [f"{i},$set,{p}" for i, p in doc["sets"]]
    engine = {"datasource": {"params": doc["datasource_params"]}, "algorithms": [{"name": "ur", "params": doc["algorithm_params"]}]}
    td = DataSource(DataSourceParams.from_engine_json(engine)).readTraining(lines)
    ap = URAlgorithmParams.from_engine_json(engine)
    ap.seed = 1
    model = URAlgorithm(ap, library=sim_lib).train(Preparator().prepare(td))     # URModel(correlators, Seq(properties))
    docs = {d["id"]: d for d in model.documents()}
    ref, _ = _oracle_model(doc, by_event)
    props = item_properties(doc["sets"])
    assert set(docs) == set(ref) | set(props)                       # full outer join of indicators and properties
    for item, d in docs.items():
        for ev in ("purchase", "view", "category-pref"):
            assert d.get(ev) == ref.get(item, {}).get(ev)
        for name, values in props.get(item, {}).items():
            assert d[name] == values
    assert docs["Iphone 4"]["view"] == ["Soap", "Tablets"] and "purchase" not in docs["Galaxy"]
    n = model.save(str(tmp_path / "model.ndjson"))
    out = [json.loads(l) for l in open(tmp_path / "model.ndjson")]
    assert n == len(docs) and len(out) == 2 * n and out[0]["index"]["_id"] == out[1]["id"]


def test_extract_jvalue_types_dates_and_ranks_before_indexing(sim_lib, tmp_path):
    """URModel.extractJvalue (URModel.scala:126-140, applied at :67-74 with URAlgorithm's dateNames, :264-267): the handmade
    engine names `available` / `expires` / `date` as date properties -- their ISO strings become dates, a ranking field that
    arrives as a string becomes a double, lists map element-wise, everything else passes through."""
    from datetime import datetime, timezone
    from universal_recommender_amd.data_source import DataSource, DataSourceParams
    from universal_recommender_amd.preparator import Preparator
    from universal_recommender_amd.ur_algorithm import URAlgorithm, URAlgorithmParams
    from universal_recommender_amd.ur_model import URModel, extractJvalue
    doc, by_event, _, items = _load("handmade.json")
    eng = {"datasource": {"params": doc["datasource_params"]}, "algorithms": [{"name": "ur", "params": dict(doc["algorithm_params"], availableDateName="available",
                                                                                                      expireDateName="expires", dateName="date")}]}
    # the committed parameters are the reference's handmade engine's (tests/golden/make_golden.py), its date names among them
    rp = doc["algorithm_params"]
    assert (rp["availableDateName"], rp["expireDateName"], rp["dateName"]) == ("available", "expires", "date")
    ap = URAlgorithmParams.from_engine_json(eng)
    ap.seed = 1
    algo = URAlgorithm(ap, library=sim_lib)
    assert algo.dateNames == ["date", "available", "expires"]
    lines = [",".join(e) for e in doc["events"]] + [f"{i},$set,{p}" for i, p in doc["sets"]]
    model = algo.train(Preparator().prepare(DataSource(DataSourceParams.from_engine_json(eng)).readTraining(lines)))
    model.propertiesMaps.append({"Iphone 4": {"available": "2016-03-02T12:00:00.000-08:00", "expires": ["2017-01-01T00:00:00Z"], "popRank": "3.5", "hotRank": 2,
                                              "defaultRank": "4.0", "title": "2016-03-02T12:00:00Z"}})
    d = {x["id"]: x for x in model.documents(algo.dateNames)}["Iphone 4"]
    assert d["available"] == datetime(2016, 3, 2, 20, 0, tzinfo=timezone.utc) and d["expires"] == [datetime(2017, 1, 1, tzinfo=timezone.utc)]
    assert d["popRank"] == 3.5 and isinstance(d["popRank"], float) and d["hotRank"] == 2
    assert d["defaultRank"] == "4.0" and d["title"] == "2016-03-02T12:00:00Z"     # neither a date name nor a ranking field: untouched
    assert d["view"] == ["Soap", "Tablets"]                                        # indicator lists are lists of strings: untouched
    plain = {x["id"]: x for x in model.documents()}["Iphone 4"]                    # no dateNames: strings stay strings, ranks still become doubles
    assert plain["available"] == "2016-03-02T12:00:00.000-08:00" and plain["popRank"] == 3.5
    assert extractJvalue(["t"], "t", [["2016-03-02"]])[0][0].year == 2016 and extractJvalue([], "n", True) is True
    model.save(str(tmp_path / "m.ndjson"), algo.dateNames)
    saved = {json.loads(l)["id"]: json.loads(l) for l in list(open(tmp_path / "m.ndjson"))[1::2]}
    assert saved["Iphone 4"]["available"] == "2016-03-02T20:00:00.000Z" and saved["Iphone 4"]["popRank"] == 3.5
