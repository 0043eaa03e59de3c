"""The quota= keyword on the host simulator over the handmade golden data (the stack of tests/test_recommend_rules_golden.py): user_recommendations and
batch_predict under a quota on the categories property equal the sequential walk of tests/quota_cases.py applied on the host to the rows of the
quota-less call with num = pool; a call without quota returns what it returned before."""
import numpy as np
import pytest

from eval_ref import bits
from test_recommend_rules_golden import NOW_MS, _stack


def _greedy(model, props, row, num, most):
    """the first num items of `row` (names) such that no category is held by more than `most` of them"""
    kept, held = [], {}
    for item in row:
        cats = set(props.get(item, {}).get("categories", []))
        if len(kept) < num and all(held.get(c, 0) < most for c in cats):
            kept.append(item)
            held.update({c: held.get(c, 0) + 1 for c in cats})
    return kept


@pytest.mark.parametrize("most,num", [(1, 3), (2, 4)])
def test_quota_is_the_walk_over_the_pool(sim_session, most, num):
    from universal_recommender_amd.history import DeviceHistory
    algo, model, _, history, *_, props = _stack(sim_session)
    dh, quota, pool = DeviceHistory.from_dict(sim_session, model, history), [{"name": "categories", "max": most}], min(model.n_items, 256)
    plain = algo.user_recommendations(model, dh, num=pool, now_ms=NOW_MS)
    assert len(plain) == 3                                                                      # without quota: the three tensors of before
    p_count, p_idx, p_score = (t.cpu().numpy() for t in plain)
    count, idx, score, short = (t.cpu().numpy() for t in algo.user_recommendations(model, dh, num=num, now_ms=NOW_MS, quota=quota, pool=pool))
    cut = 0
    for u in range(dh.n_users):
        row = [model.item_name(int(i)) for i in p_idx[u, : p_count[u]]]
        want = _greedy(model, props, row, num, most)
        cut += want != row[:num]
        assert [model.item_name(int(i)) for i in idx[u, : count[u]]] == want and short[u] == (len(want) < num and p_count[u] == pool), u
        assert bits(score[u, : count[u]]).tolist() == [bits(p_score[u, row.index(i)])[0] for i in want]
    assert cut                                                                                  # the quota moved a row at least
    users = sorted(history)[:3]
    queries = [{"user": u} for u in users] + [{"user": users[0], "num": num + 1, "quota": [{"name": "categories", "max": 1}]}, {"user": users[0], "quota": []}]
    base = algo.batch_predict(model, [dict(q, num=pool) for q in queries[:3]], dh, now_ms=NOW_MS)
    got = algo.batch_predict(model, [dict(q, num=q.get("num", num)) for q in queries], dh, now_ms=NOW_MS, quota=quota, pool=pool)
    rows = [[s["item"] for s in b["itemScores"]] for b in base]
    for g, row, (n, m) in zip(got, rows + rows[:1] * 2, [(num, most)] * 3 + [(num + 1, 1), (num, None)]):
        assert [s["item"] for s in g["itemScores"]] == (row[:n] if m is None else _greedy(model, props, row, n, m))
    with pytest.raises(ValueError, match="colour"):
        algo.user_recommendations(model, dh, quota=[{"name": "colour", "max": 1}])
