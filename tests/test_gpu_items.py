"""urcco_dev_item_bounds / _rows on the MI355X against the numpy restatement of decision D18 (tests/items_ref.py): the problem and the checks of
tests/test_sim_items.py -- every class boundary lies inside its 320 items, so no larger shape is needed -- and similar_items against batch_predict
on a device-built model."""
import numpy as np
import pytest
import torch

import history_ref as H
import items_ref as I

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu_session):
    return I.DeviceProblem(gpu_session, I.make_problem())


@pytest.mark.parametrize("cap", I.CAPS)
def test_rows_match_the_restatement(dev, cap):
    stats, rows = I.check(dev, [cap] * 3)
    assert stats[0] + stats[1] + stats[2] == dev.p.q_items.size * 3 and stats[0] > 0, stats
    assert (stats[1] > 0) == (cap >= 65) and (stats[2] > 0) == (cap >= 4097) and (stats[3] > 0) == (cap < I.LONGEST), stats
    _, again = I.check(dev, [cap] * 3)                       # and from run to run
    assert all(np.array_equal(x, y) for a, b in zip(rows, again) for x, y in zip(a, b))


def test_mixed_caps(dev):
    stats, _ = I.check(dev, [6000, 2, 65])
    assert stats[0] > 0 and stats[1] > 0 and stats[2] > 0 and stats[3] > 0, stats
    I.check(dev, [1, 4097, 100])


@pytest.mark.parametrize("cap", (64, 100, 6000))
def test_capacity_below_the_bounds(dev, cap):
    I.capacity_cases(dev, [cap] * 3)


def test_similar_items_against_batch_predict(gpu_session):
    """400 items, two event types, integer ids: the table in chunks of 64 (a ragged last one) equals batch_predict's answers to {"item": x} on both
    routes, with and without return_self and with the lists as a filter (item_bias < 0); the result stays on the device"""
    algo, model = H.predict_stack(gpu_session, 3000, 400, 250)
    names = list(range(model.n_items)) + [400, -3]
    for kw in ({}, {"return_self": True}, {"item_bias": -1.0, "num": 5}, {"item_bias": 2.5}):
        q_kw = {k2: kw[k] for k, k2 in (("num", "num"), ("item_bias", "itemBias"), ("return_self", "returnSelf")) if k in kw}
        qs = [dict(q_kw, item=x) for x in names]
        want = algo.batch_predict(model, qs, {})
        assert algo.batch_predict(model, qs, {}, item_rows="device") == want
        count, idx, score = algo.similar_items(model, names, chunk=64, **kw)
        assert count.is_cuda and idx.is_cuda and score.is_cuda
        count, idx, score = count.cpu().numpy(), idx.cpu().numpy(), score.cpu().numpy()
        for r, w in enumerate(want):
            assert [{"item": int(idx[r, j]), "score": float(score[r, j])} for j in range(int(count[r]))] == w["itemScores"], (kw, names[r])
    assert any(s["score"] > 0 for r in want for s in r["itemScores"])
    whole = algo.similar_items(model)
    part = algo.similar_items(model, torch.arange(model.n_items, dtype=torch.int32, device=gpu_session.device), chunk=100)
    assert all(torch.equal(a, b) for a, b in zip(whole, part))
