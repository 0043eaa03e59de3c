"""The diversify= keyword on the host simulator over the handmade golden data (the stack of tests/test_recommend_rules_golden.py): user_recommendations and
batch_predict under a penalty equal the greedy MMR rule of tests/diversify_cases.py applied on the host to the rows of the plain call with num = pool; with a
quota in the same call the re-ranked pool is cut by the walk of tests/quota_cases.py; diversify=0 returns what the call returned before."""
import numpy as np

import diversify_cases as D
import quota_cases as Q
from eval_ref import bits
from test_recommend_rules_golden import NOW_MS, _stack
from universal_recommender_amd import _lib


def test_diversify_is_the_rule_over_the_pool(sim_session):
    from universal_recommender_amd.history import DeviceHistory
    algo, model, _, history, *_ = _stack(sim_session)
    dh, n, pool, num, pen = DeviceHistory.from_dict(sim_session, model, history), model.n_items, min(model.n_items, 256), 4, 0.5
    rows_of = lambda m: (lambda rp, ci: [ci[rp[i]:rp[i + 1]] for i in range(n)])(m.row_ptr.cpu().numpy(), m.col_idx.cpu().numpy())
    sim, cats = rows_of(model.correlators[0]), rows_of(model.properties["categories"])
    call = lambda **kw: [t.cpu().numpy() for t in algo.user_recommendations(model, dh, now_ms=NOW_MS, **kw)]
    count, idx, score = call(num=pool)
    for a, b in zip(call(num=num), call(num=num, diversify=0)):                                  # off: today's tensors
        assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
    want = D.mmr(dict(count=count, idx=idx, score=score, sim=sim, num=num, penalty=pen), n)
    got = call(num=num, diversify=pen, pool=pool)
    assert len(got) == 3 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(bits(got[2]).reshape(want[2].shape), want[2])
    assert not np.array_equal(want[1], idx[:, :num])                                            # the penalty moved a row at least
    full = D.mmr(dict(count=count, idx=idx, score=score, sim=sim, num=pool, penalty=pen), n)
    cut = Q.walk(dict(count=full[0], idx=full[1], score=full[2].view(np.float64), rules=[(cats, 1)], num=num, slots=_lib.QUOTA_LDS_SLOTS))   # the whole pool re-ranked, that order cut
    got = call(num=num, diversify=pen, pool=pool, quota=[{"name": "categories", "max": 1}])
    assert len(got) == 4 and all(np.array_equal(bits(g).reshape(w.shape) if g.dtype == np.float64 else g, w) for g, w in zip(got, cut[:4]))
    user, ids = sorted(history)[0], {model.item_name(i): i for i in range(n)}                    # batch_predict: one query carries its own key, the other stays as it was
    base = algo.batch_predict(model, [{"user": user, "num": pool}], dh, now_ms=NOW_MS)[0]["itemScores"]
    row = dict(count=np.array([len(base)], np.int32), idx=np.array([[ids[s["item"]] for s in base]], np.int32), score=np.array([[s["score"] for s in base]]))
    want = D.mmr(dict(row, sim=sim, num=num, penalty=pen), n)
    got = algo.batch_predict(model, [{"user": user, "num": num}, {"user": user, "num": num, "diversify": pen}], dh, now_ms=NOW_MS, pool=pool)
    assert got[0]["itemScores"] == base[:num]
    assert [(ids[s["item"]], s["score"]) for s in got[1]["itemScores"]] == [(int(i), float(row["score"][0, p])) for i, p in zip(want[1][0, : want[0][0]], want[3][0])]
