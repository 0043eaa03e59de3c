"""list_metrics on the host simulator over the handmade golden data: the metrics of user_recommendations' table, with and without quota=, equal the definitions
of tests/list_metrics_cases.py; evaluate(list_metrics=True) reports the same numbers for every chunk, and evaluate() without it the keys it returned before."""
import numpy as np

import list_metrics_cases as L
from eval_ref import bits
from test_recommend_rules_golden import NOW_MS, _stack

KS, FLOATS = (1, 3, 5), ("coverage", "gini", "herfindahl", "ils", "novelty")


def test_list_metrics_of_a_table_and_of_evaluate(sim_session):
    from universal_recommender_amd.history import DeviceHistory
    algo, model, _, history, *_ = _stack(sim_session)
    dh, n, sim = DeviceHistory.from_dict(sim_session, model, history), model.n_items, model.correlators[0]
    rp, ci = sim.row_ptr.cpu().numpy(), sim.col_idx.cpu().numpy()
    rows, pop, reports = [ci[rp[i]:rp[i + 1]] for i in range(n)], np.arange(n) % 4, []
    for kw in ({}, {"quota": [{"name": "categories", "max": 1}], "pool": min(n, 256)}):
        count, idx = algo.user_recommendations(model, dh, num=KS[-1], now_ms=NOW_MS, **kw)[:2]
        p = dict(count=count.cpu().numpy(), idx=idx.cpu().numpy(), num=KS[-1], ks=KS, sim=rows)
        got = algo.list_metrics(model, count, idx, KS, popularity=pop, chunk=2)
        bucket, (linked, _) = L.exposure_ref(p, n), L.links_ref(p, n)
        expo, stats = L.stats_ref(bucket)
        assert np.array_equal(got["bucket"].cpu().numpy(), bucket) and np.array_equal(got["per_user"]["linked"].cpu().numpy(), linked)
        for key, w in L.floats_ref(p, stats, expo, linked, pop, n).items():
            assert bits(np.array(got[key])).tolist() == bits(np.array(w)).tolist(), (kw, key)
        reports.append(got)
    assert reports[0]["total"][-1] > 0 and any(reports[0][k] != reports[1][k] for k in FLOATS)   # the quota moved a metric at least
    plain = algo.evaluate(model, dh, dh, ks=KS, now_ms=NOW_MS)
    assert sorted(plain) == ["evaluated", "hit_rate", "ks", "map", "ndcg", "not_evaluated", "per_user", "precision"] and sorted(plain["per_user"]) == ["ap", "hits", "ndcg"]
    for chunk in (7, 65536):
        got = algo.evaluate(model, dh, dh, ks=KS, now_ms=NOW_MS, chunk=chunk, list_metrics=True, popularity=pop)
        assert all(got[k] == plain[k] for k in ("map", "ndcg", "precision", "hit_rate")) and sorted(got["per_user"]) == ["ap", "hits", "linked", "ndcg"]
        for key in FLOATS + ("covered", "total"):
            assert bits(np.array(got[key], np.float64)).tolist() == bits(np.array(reports[0][key], np.float64)).tolist(), (chunk, key)
