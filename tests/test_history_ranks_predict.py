"""DeviceHistory.ranks, DeviceModel.set_ranks, URAlgorithm.ranks_from_history and train_from_history(ranks="history") (decision D24) on the simulator
session: the rank fields of a resident history are those of the PopModel restatement (oracle.cco_oracle.get_ranks) over the same events, restricted to
the items of the primary's dictionary; the backfill they give answers queries in the order of the multi-field tuple sort; they follow append and trim;
a retrained model carries them; the ValueErrors."""
import datetime

import numpy as np
import pytest
import torch

import history_matrix_cases as M
import test_pop_model as TP
from oracle import cco_oracle as PO
from universal_recommender_amd import _lib

NONE = _lib.RANK_NONE
DAY = 86_400_000
NOW = 1_790_000_000_000


def history_of(sess, model, rows, user_ids=None):
    """rows of (user, event name, item, time ms) -> DeviceHistory: dense user ids by first appearance, item ids in the event type's column dictionary
    (the primary's for an event outside the model), -1 outside it"""
    from universal_recommender_amd.history import DeviceHistory
    user_ids = {} if user_ids is None else user_ids
    per = {}
    for u, ev, it, t in rows:
        c = model.by_name.get(ev)
        i = model.column_index(c, it) if c is not None else model.item_index(it)
        per.setdefault(ev, []).append((user_ids.setdefault(u, len(user_ids)), -1 if i is None else i, t))
    return DeviceHistory.from_streams(sess, model, streams_of(sess, per), user_ids=user_ids), per


def streams_of(sess, per):
    return {ev: (torch.tensor([r[0] for r in rs], dtype=torch.int32).to(sess.device), torch.tensor([r[1] for r in rs], dtype=torch.int32).to(sess.device),
                 torch.tensor([r[2] for r in rs], dtype=torch.int64).to(sess.device)) for ev, rs in per.items()}


def as_dict(model, fields):
    """{field: tensor} -> item -> {field: rank} over the items that have one: the form of get_ranks"""
    out = {}
    for f, t in fields.items():
        assert t.dtype == torch.int64 and t.numel() == model.n_items
        for i, v in enumerate(t.cpu().tolist()):
            if v != NONE:
                out.setdefault(model.item_name(i), {})[f] = float(v)
    return out


def restricted(model, ref):
    return {i: r for i, r in ref.items() if model.item_index(i) is not None}


def tuple_order(fields, n_items):
    """the multi-field sort in plain Python: every field descending, an item without a rank last, then the item index"""
    cols = [t.cpu().tolist() for t in fields.values()]
    return sorted(range(n_items), key=lambda i: tuple((1, 0) if c[i] == NONE else (0, -c[i]) for c in cols) + (i,))


# ---- the reference's rank data --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(sim_session):
    from universal_recommender_amd.data_source import DataSource, DataSourceParams
    from universal_recommender_amd.preparator import Preparator
    from universal_recommender_amd.recommend import DeviceModel
    from universal_recommender_amd.ur_algorithm import URAlgorithm, URAlgorithmParams
    d, events, now = TP._rank_fixture()
    engine = {"datasource": {"params": {"appName": "default-rank", "eventNames": d["eventNames"]}},
              "algorithms": [{"name": "ur", "params": {"appName": "default-rank", "indexName": "urindex", "typeName": "items", "recsModel": "all",
                                                       "eventNames": d["eventNames"], "rankings": d["rankings"], "numGPUs": 1}}]}
    td = DataSource(DataSourceParams.from_engine_json(engine)).readTraining([f"{e[0]},{e[1]},{e[2]}" for e in d["events"]])
    ap = URAlgorithmParams.from_engine_json(engine)
    ap.seed = 3
    algo = URAlgorithm(ap, device=0, library=sim_session.lib, sess=sim_session)
    model = DeviceModel.from_indicators(sim_session, algo.train(Preparator().prepare(td)).coocurrenceMatrices)
    dh, _ = history_of(sim_session, model, [(e[0], e[1], e[2], t) for e, (_, _, t) in zip(d["events"], events)])
    return d, events, now, algo, model, dh


def test_golden_rank_fields_are_the_oracle_s(golden):
    d, events, now, algo, model, dh = golden
    rankings = [{"name": "popularRank", "type": "popular", "eventNames": ["show", "like"], "duration_s": 3650 * 86400}, {"name": "defaultRank", "type": "userDefined"}]
    fields = dh.ranks(rankings, now_ms=now + 1, model_event_names=d["eventNames"])
    assert list(fields) == ["popularRank", "defaultRank"] and bool((fields["defaultRank"] == NONE).all())
    ref = restricted(model, PO.get_ranks(rankings, events, d["eventNames"], now + 1))
    assert as_dict(model, fields) == ref and len(ref) >= 4 and all(set(r) == {"popularRank"} for r in ref.values())
    # the default names and event names: popRank over the primary
    assert as_dict(model, dh.ranks([{}], now_ms=now + 1, model_event_names=d["eventNames"])) == restricted(model, PO.get_ranks([{}], events, d["eventNames"], now + 1))
    assert list(dh.ranks([{"type": "nonsense"}, {"type": "hot"}], now_ms=now + 1)) == ["unknownRank", "hotRank"]


def test_golden_pure_backfill_order(golden):
    """what test_pop_model.test_oracle_popular_order_matches_the_reference_golden asserts of popular_order_expected, of batch_predict's pure backfill"""
    d, events, now, algo, model, dh = golden
    r = [x for x in d["rankings"] if x["type"] == "popular"][0]
    fields = dh.ranks([{"name": r["name"], "type": "popular", "eventNames": r["eventNames"], "duration_s": 3650 * 86400}], now_ms=now + 1)
    model.set_ranks(fields)
    try:
        res = algo.batch_predict(model, [{"num": 20}], dh)[0]["itemScores"]
    finally:
        model.set_ranks({})
    order = [s["item"] for s in res]
    ranks = restricted(model, {i: v for i, v in PO.pop_calc("popular", events, r["eventNames"], 3650 * 86400, now + 1).items()})
    counts = [ranks.get(i, 0.0) for i in order]
    assert sorted(order) == sorted(model.item_name(i) for i in range(model.n_items)) and all(s["score"] == 0 for s in res)
    assert counts == sorted(counts, reverse=True) and counts[0] == 6.0 and counts[1] == 5.0
    assert set(order[: len(ranks)]) == set(ranks) and all(c == 0.0 for c in counts[len(ranks):])
    assert [x for x in d["popular_order_expected"] if x in ranks][:2] == order[:2]


def test_random_is_not_served_and_a_history_needs_its_model(golden, sim_session):
    from universal_recommender_amd.history import DeviceHistory
    d, events, now, algo, model, dh = golden
    assert [r.type for r in algo.rankingsParams] == ["popular", "userDefined", "random"]
    with pytest.raises(ValueError, match="random"):
        algo.ranks_from_history(dh, now + 1)
    with pytest.raises(ValueError, match="random"):
        dh.ranks([{"type": "popular"}, {"type": "random"}], now_ms=now + 1)
    with pytest.raises(ValueError, match="model"):
        DeviceHistory(sim_session, dh.n_users, dh.user_ids, dh.types, None).ranks([{}], now_ms=now + 1)
    untimed = DeviceHistory.from_streams(sim_session, model, {"show": (torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), None)}, n_users=1)
    with pytest.raises(ValueError, match="times"):
        untimed.ranks([{}], now_ms=now + 1)


# ---- a synthetic timed history: three event types, one with a column dictionary of its own -----------------------------------------------------------
N_ITEMS, N_VIEW, N_USERS = 60, 40, 50
RANKINGS = [{"name": "buyRank", "type": "popular", "eventNames": ["purchase", "like"], "duration_s": 20 * 86400},
            {"type": "trending", "eventNames": ["view"], "duration_s": 10 * 86400, "end_ms": NOW - DAY},
            {"type": "hot", "duration_s": 12 * 86400},
            {"name": "allRank", "type": "popular", "eventNames": [], "duration_s": 5 * 86400 + 1}]


def make_rows(seed, n):
    rng = np.random.default_rng(seed)
    view_names = view_dictionary()
    rows = []
    for _ in range(n):
        ev = str(rng.choice(["purchase", "view", "like"], p=[0.4, 0.4, 0.2]))
        z = int(min(rng.zipf(1.4), 70)) - 1
        # a view names a column of its own dictionary (30 of them items of the primary, in another order; 10 not) or, like i60 .. i69 of the others, nothing known
        item = (view_names[z % len(view_names)] if z < 45 else f"y{z}") if ev == "view" else f"i{z}"
        rows.append((f"u{int(rng.integers(0, N_USERS))}", ev, item, int(NOW - rng.integers(0, 30 * DAY))))
    return rows


def view_dictionary():
    rng = np.random.default_rng(2)
    return [str(x) for x in rng.permutation([f"i{k}" for k in rng.permutation(N_ITEMS)[:30]] + [f"x{k}" for k in range(N_VIEW - 30)])]


@pytest.fixture(scope="module")
def stack(sim_session):
    from helpers import rand_csr, run_device
    from oracle import c_oracle as O
    from universal_recommender_amd.indexed_dataset import BiDictionary
    from universal_recommender_amd.recommend import DeviceModel
    from universal_recommender_amd.ur_algorithm import RankingParams, URAlgorithm, URAlgorithmParams
    sess = sim_session
    rng = np.random.default_rng(31)
    out = run_device(sess, [rand_csr(rng, 400, N_ITEMS, 8), rand_csr(rng, 400, N_VIEW, 10)], [O.DatasetParams(100, 20, None)] * 2, 7)
    item_ids = BiDictionary([f"i{k}" for k in range(N_ITEMS)])
    model = DeviceModel.from_indicators(sess, [("purchase", out[0]), ("view", out[1])], item_ids=item_ids,
                                        column_ids={"purchase": item_ids, "view": BiDictionary(view_dictionary())}, properties={})
    engine = {"algorithms": [{"name": "ur", "params": {"appName": "t", "indexName": "t", "typeName": "items", "num": 10,
                                                       "indicators": [{"name": "purchase", "maxItemsPerUser": 6}, {"name": "view", "maxItemsPerUser": 70}]}}]}
    algo = URAlgorithm(URAlgorithmParams.from_engine_json(engine), device=0, library=sess.lib)
    algo.ap.seed = 11
    iso = datetime.datetime.fromtimestamp((NOW - DAY) / 1000, datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%S.000Z")
    algo.ap.rankings = [RankingParams("buyRank", "popular", ["purchase", "like"], None, None, "20 days"), RankingParams(None, "trending", ["view"], iso, None, "10 days"),
                        RankingParams(None, "hot", None, None, None, "12 days")]
    rows = make_rows(7, 4000) + [("short", "purchase", "i5", NOW - DAY)]      # a user with a one-event history
    dh, per = history_of(sess, model, rows)
    assert dh.types["view"].col_map is not None and dh.types["purchase"].col_map is None and dh.types["like"].col_map is None and dh.types["like"].n_cols == N_ITEMS
    cmap = dh.types["view"].col_map.cpu().numpy()
    assert (cmap < 0).sum() == N_VIEW - 30 and not np.array_equal(cmap[cmap >= 0], np.sort(cmap[cmap >= 0]))
    return algo, model, dh, rows, per


def oracle_events(rows):
    return [(ev, it, t) for _, ev, it, t in rows]


def same_fields(a, b):
    return list(a) == list(b) and all(torch.equal(a[f].cpu(), b[f].cpu()) for f in a)


def test_synthetic_rank_fields_are_the_oracle_s(stack):
    algo, model, dh, rows, per = stack
    fields = dh.ranks(RANKINGS, now_ms=NOW, model_event_names=["purchase", "view"])
    assert list(fields) == ["buyRank", "trendRank", "hotRank", "allRank"]
    ref = restricted(model, PO.get_ranks(RANKINGS, oracle_events(rows), ["purchase", "view"], NOW))
    got = as_dict(model, fields)
    assert got == ref
    for f in fields:
        assert sum(f in r for r in ref.values()) >= 5, f
    assert any(r.get("trendRank", 0) < 0 for r in ref.values()) and any(r.get("hotRank", 0) != 0 for r in ref.values())
    # a name the history does not hold contributes nothing; the mapping of the algorithm's rankings is getRanks' own
    with_unknown = [dict(RANKINGS[0], eventNames=["purchase", "no such event", "like"])]
    assert torch.equal(dh.ranks(with_unknown, now_ms=NOW)["buyRank"].cpu(), fields["buyRank"].cpu())
    from_algo = algo.ranks_from_history(dh, NOW)
    assert same_fields(from_algo, {f: fields[f] for f in ("buyRank", "trendRank", "hotRank")})


def test_set_ranks_orders_the_backfill_by_every_field(stack):
    algo, model, dh, rows, per = stack
    fields = dh.ranks(RANKINGS[1:3] + RANKINGS[:1], now_ms=NOW, model_event_names=["purchase", "view"])      # trendRank, hotRank, buyRank: the early fields tie and miss often
    want = tuple_order(fields, model.n_items)
    assert want != tuple_order({"b": fields["buyRank"]}, model.n_items) and want != list(range(model.n_items))
    assert model.set_ranks(fields) is model
    try:
        assert model.fill_order.cpu().tolist() == want and list(model.rank_fields) == ["trendRank", "hotRank", "buyRank"]
        res = algo.batch_predict(model, [{"num": model.n_items}], dh)[0]["itemScores"]
        assert [s["item"] for s in res] == [model.item_name(i) for i in want] and all(s["score"] == 0 for s in res)
        # a user with a short history: the scored items first, ties and the rest in backfill order
        res = algo.batch_predict(model, [{"user": "short", "num": model.n_items}], dh)[0]["itemScores"]
        place = {model.item_name(i): p for p, i in enumerate(want)}
        keys = [(-s["score"], place[s["item"]]) for s in res]
        assert keys == sorted(keys) and len(set(s["item"] for s in res)) == len(res) > 10
        assert res[0]["score"] > 0 and res[-1]["score"] == 0
    finally:
        assert model.set_ranks({}).fill_order is None and model.rank_fields == {}
    with pytest.raises(ValueError):
        model.set_ranks({"short": fields["buyRank"][:-1]})
    with pytest.raises(ValueError):
        model.set_ranks({"float": fields["buyRank"].to(torch.float64)})


def test_ranks_follow_append_and_trim(sim_session, stack):
    from universal_recommender_amd.history import DeviceHistory
    algo, model, dh, rows, per = stack
    at = len(rows) * 2 // 3
    user_ids = dict(dh.user_ids)
    part, _ = history_of(sim_session, model, rows[:at], {u: i for u, i in user_ids.items()})
    _, tail = history_of(sim_session, model, rows[at:], {u: i for u, i in user_ids.items()})
    part.append(streams_of(sim_session, tail), n_users=len(user_ids))
    whole = dh.ranks(RANKINGS, now_ms=NOW, model_event_names=["purchase", "view"])
    assert same_fields(part.ranks(RANKINGS, now_ms=NOW, model_event_names=["purchase", "view"]), whole)
    cut, drop = NOW - 8 * DAY, ["u3", "u10", "u41"]
    part.trim(before_ms=cut, drop_users=drop)
    left = [r for r in rows if r[3] >= cut and r[0] not in drop]
    assert 0 < len(left) < len(rows)
    filtered, _ = history_of(sim_session, model, left, {u: i for u, i in user_ids.items()})
    got = part.ranks(RANKINGS, now_ms=NOW, model_event_names=["purchase", "view"])
    assert same_fields(got, filtered.ranks(RANKINGS, now_ms=NOW, model_event_names=["purchase", "view"])) and not same_fields(got, whole)
    assert as_dict(model, got) == restricted(model, PO.get_ranks(RANKINGS, oracle_events(left), ["purchase", "view"], NOW))


def test_train_from_history_with_ranks_from_the_history(stack):
    algo, model, dh, rows, per = stack
    new = algo.train_from_history(dh, ranks="history", now_ms=NOW)
    base = algo.train_from_history(dh)
    assert base.fill_order is model.fill_order and base.rank_fields is model.rank_fields and base.properties is model.properties      # ranks=None: the old order
    fields = algo.ranks_from_history(dh, NOW)
    base.set_ranks(fields)
    assert list(new.rank_fields) == ["buyRank", "trendRank", "hotRank"] and same_fields(new.rank_fields, fields)
    assert torch.equal(new.fill_order.cpu(), base.fill_order.cpu()) and new.fill_order.cpu().tolist() == tuple_order(fields, model.n_items)
    assert M.same_model(new, base) and new.properties is model.properties and new.dates is model.dates and model.fill_order is None
    given = algo.train_from_history(dh, ranks="history", now_ms=NOW, properties={"i3": {"color": ["red"]}}, date_names=())
    assert "color" in given.properties and torch.equal(given.fill_order.cpu(), new.fill_order.cpu())
    with pytest.raises(ValueError):
        algo.train_from_history(dh, ranks="popular")
    as_before = algo.train_from_history(dh, ranks={"i4": 1.0})
    assert int(as_before.fill_order[0]) == 4 and as_before.rank_fields == {}
