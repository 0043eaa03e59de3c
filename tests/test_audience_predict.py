"""URAlgorithm.audience on the host simulator over the handmade golden data (the stack of tests/test_recommend_rules_golden.py): every returned (user,
item, score) is the score user_recommendations(num = the catalogue) gives that item in that user's row, bit for bit; every user with a positive score for
the item is in its audience, in the order (score desc, user index asc); user chunks of 2 give the same tensors."""
import numpy as np
import pytest
import torch

from test_recommend_rules_golden import _stack


def test_audience_is_the_transposed_user_table(sim_session):
    from universal_recommender_amd.history import DeviceHistory
    algo, model, _, history, *_ = _stack(sim_session, with_properties=False)
    items = [model.item_name(i) for i in range(model.n_items)]
    algo.recsModel = "collabFiltering"                                                          # no backfill: the table holds the positive scores alone
    dh = DeviceHistory.from_dict(sim_session, model, history)
    assert model.n_items <= 256
    r_count, r_idx, r_score = (t.cpu().numpy() for t in algo.user_recommendations(model, dh, num=model.n_items))
    table = {(u, int(r_idx[u, j])): r_score[u, j] for u in range(dh.n_users) for j in range(int(r_count[u]))}
    assert table
    count, user, score = algo.audience(model, dh, items + items[:1], num=dh.n_users + 1)
    again = algo.audience(model, dh, items + items[:1], num=dh.n_users + 1, user_chunk=2)
    assert all(torch.equal(a, b) for a, b in zip((count, user, score), again))
    count, user, score = (t.cpu().numpy() for t in (count, user, score))
    for x, item in enumerate(items + items[:1]):
        i = model.item_index(item)
        want = sorted((-s, u) for (u, it), s in table.items() if it == i)
        got = [(-score[x, r], int(user[x, r])) for r in range(int(count[x]))]
        assert [(np.float64(s).view(np.int64), u) for s, u in want] == [(np.float64(s).view(np.int64), u) for s, u in got], item
    assert count.sum() == 2 * sum(1 for (u, it) in table if it == model.item_index(items[0])) + sum(1 for (u, it) in table if it != model.item_index(items[0]))
    top = algo.audience(model, dh, torch.tensor([model.item_index(items[0])], dtype=torch.int32), num=1)
    assert int(top[0][0]) == min(1, int(count[0])) and (int(count[0]) == 0 or int(top[1][0, 0]) == int(user[0, 0]))
    with pytest.raises(ValueError):
        algo.audience(model, dh, ["no such item"])
