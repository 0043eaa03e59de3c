"""urcco_dev_history_* on the MI355X against the numpy restatement of decision D17 (tests/history_ref.py): the problem and the checks of
tests/test_sim_history.py, one larger shape, and batch_predict with a DeviceHistory against batch_predict with the dict.

The keys of the select, by byte, as in tests/test_sim_history.py: every time byte 0..7 alone, two bytes around uniform ones, the whole int64 domain and
equal times (make_key_problem); the top position byte with a real index over 2^24 + 2^16 events (make_far_problem).  The capacity clause of
include/urcco.h runs with 256 sentinel entries behind every buffer; DeviceHistory.from_streams with real times runs against the dict form."""
import numpy as np
import pytest
import torch

import history_ref as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def problem():
    return H.make_problem()


@pytest.fixture(scope="module")
def dev(gpu_session, problem):
    return H.DeviceProblem(gpu_session, problem)


def test_index_holds_every_users_positions(dev):
    for s, (_, rp, pos, *_rest) in zip(dev.p.streams, dev.ev):
        rp, rows = H.csr_rows(rp, pos)
        assert rp[-1] == np.count_nonzero(s.users >= 0)
        for u, r in enumerate(rows):
            assert np.array_equal(np.sort(r), np.flatnonzero(s.users == u))


@pytest.mark.parametrize("cap", H.CAPS)
def test_rows_match_the_restatement(dev, cap):
    stats, _, _ = H.check(dev, [cap] * 3)
    assert stats[0] + stats[1] + stats[2] == dev.p.q_users.size * 3 and stats[0] > 0 and stats[1] > 0 and stats[2] > 0, stats
    assert (stats[3] > 0) == (cap < H.HEAVY) and stats[4] > 0 and stats[5] > 0, stats


def test_mixed_caps_no_blacklist_no_extra(dev):
    H.check(dev, [100, 1, 3])
    H.check(dev, [5, 5, 5], use_extra=False, blacklist=[False] * 3)
    H.check(dev, [5, 64, 5000], use_extra=False, blacklist=[False, False, True])


def test_rows_do_not_depend_on_the_order_inside_the_index(gpu_session, problem, dev):
    other = H.DeviceProblem(gpu_session, problem, shuffle_index_seed=3)
    for cap in (5, 100):
        _, terms_a, excl_a = H.check(dev, [cap] * 3)
        _, terms_b, excl_b = H.check(other, [cap] * 3)
        _, terms_c, excl_c = H.check(dev, [cap] * 3)          # and from run to run
        for ra, rb, rc in zip(terms_a + [excl_a], terms_b + [excl_b], terms_c + [excl_c]):
            assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(ra, rb, rc))


@pytest.fixture(scope="module")
def key_problem():
    return H.make_key_problem()


@pytest.fixture(scope="module")
def key_dev(gpu_session, key_problem):
    return H.DeviceProblem(gpu_session, key_problem)


@pytest.mark.parametrize("cap", H.KEY_CAPS)
def test_key_domain_rows_match_the_restatement(key_dev, cap):
    stats, _, _ = H.check(key_dev, [cap, cap])
    assert stats[0] > 0 and stats[1] > 0 and stats[2] > 0 and stats[3] > 0, stats


def test_key_domain_rows_do_not_depend_on_the_index_order_or_the_job_before(gpu_session, key_problem, key_dev):
    H.assert_key_edge_cases(key_problem)
    other = H.DeviceProblem(gpu_session, key_problem, shuffle_index_seed=4)
    byte0 = H.DeviceProblem(gpu_session, H.make_byte0_job())
    for cap in (20, 150, 2048):
        _, terms_a, excl_a = H.check(key_dev, [cap, 7])
        stats, _, _ = H.check(byte0, [100])           # one job whose keys differ in the lowest time byte alone, between two runs over every byte
        assert stats[1] == 1 and stats[3] == 1 and stats[0] + stats[2] == 0, stats
        _, terms_b, excl_b = H.check(other, [cap, 7])
        for ra, rb in zip(terms_a + [excl_a], terms_b + [excl_b]):
            assert all(np.array_equal(x, y) for x, y in zip(ra, rb))


def test_positions_beyond_2_24(gpu_session):
    """One stream of 2^24 + 2^16 events indexed on the device; the five users' segments against np.flatnonzero, the rows (no times / equal times: the
    top position digit decides) against the restatement over those users' events; caps below, at and above each user's events at or above 2^24."""
    p = H.make_far_problem()
    d = H.DeviceProblem(gpu_session, p, subset=range(p.n_users))
    for s, (_, rp, pos, *_rest) in zip(p.streams, d.ev):
        rp, rows = H.csr_rows(rp, pos)
        assert rp[-1] == sum(n for n, _ in H.FAR_USERS) + 4 and rows[len(H.FAR_USERS)].size == 0
        for u in range(len(H.FAR_USERS)):
            assert np.array_equal(np.sort(rows[u]), d.by_user[0][u][::-1])       # without times: most recent first = positions descending
    for cap in H.far_caps(p):
        stats, terms, _ = H.check(d, [cap, cap])
        assert stats[0] > 0 and stats[1] > 0 and stats[2] > 0 and stats[3] > 0, stats
        assert np.array_equal(terms[0][3], terms[1][3])


@pytest.mark.parametrize("cap", (5, 100))
def test_capacity_below_the_bounds(dev, cap):
    """256 sentinel entries behind every capacity: none is written."""
    H.capacity_cases(dev, [cap] * 3, pad=256)


def test_larger_shape(gpu_session):
    """20 000 users, 2 M events, one user with 300 000 of them, cap 500; 2 000 sampled queries (the heavy user among them)."""
    rng = np.random.default_rng(17)
    n_users, n_events, heavy, n_cols = 20000, 2_000_000, 300_000, 5000
    users = rng.integers(1, n_users, n_events).astype(np.int32)
    users[rng.permutation(n_events)[:heavy]] = 0
    items = rng.integers(0, n_cols, n_events).astype(np.int32)
    items[rng.random(n_events) < 0.15] = -1
    times = (1_600_000_000_000 + rng.integers(0, 86_400_000, n_events)).astype(np.int64)
    q_users = np.concatenate([[0], rng.integers(0, n_users, 1999)]).astype(np.int32)
    p = H.Problem(n_users, n_cols, [H.Stream(n_cols, users, items, times, None, True)], q_users, np.zeros(q_users.size + 1, np.int64), np.zeros(0, np.int32))
    stats, terms, excl = H.check(H.DeviceProblem(gpu_session, p), [500])
    assert stats[2] >= 1 and stats[3] >= 1 and stats[5] >= 1, stats
    assert terms[0][0].size <= 500 and excl[0].size == np.unique(items[(users == 0) & (items >= 0)]).size


def test_batch_predict_dict_against_device_history(gpu_session):
    """End to end on a device-built model (400 items, two event types, integer ids): batch_predict with the history on the device returns the items and
    scores it returns with the dict, user / user + item / userBias < 0 / blacklistItems / from + num in one batch."""
    from helpers import rand_csr, run_device
    from oracle import c_oracle as O
    from universal_recommender_amd.history import DeviceHistory
    from universal_recommender_amd.recommend import DeviceModel
    from universal_recommender_amd.ur_algorithm import URAlgorithm, URAlgorithmParams
    rng = np.random.default_rng(31)
    mats = [rand_csr(rng, 3000, 400, 8), rand_csr(rng, 3000, 250, 10)]
    out = run_device(gpu_session, mats, [O.DatasetParams(100, 20, None)] * 2, 7)
    model = DeviceModel.from_indicators(gpu_session, [("purchase", out[0]), ("view", out[1])], properties={})
    engine = {"algorithms": [{"name": "ur", "params": {"appName": "t", "indexName": "t", "typeName": "items", "num": 10,
                                                       "indicators": [{"name": "purchase", "maxItemsPerUser": 6}, {"name": "view", "maxItemsPerUser": 70}]}}]}
    algo = URAlgorithm(URAlgorithmParams.from_engine_json(engine), device=0, library=gpu_session.lib)
    history = {}
    for u in range(200):   # 0-150 events per type: below and above both caps, beyond one wave
        history[u] = {"purchase": rng.integers(0, 420, rng.integers(0, 150)).tolist(), "view": rng.integers(0, 250, rng.integers(0, 150)).tolist()}
    dh = DeviceHistory.from_dict(gpu_session, model, history)
    qs = [{"user": u} for u in range(0, 200, 3)] + [{"user": u, "item": int(u * 2)} for u in range(1, 200, 7)]
    qs += [{"user": u, "userBias": -1.0, "num": 5} for u in range(2, 60, 5)] + [{"user": u, "blacklistItems": [1, 2, 3], "from": 2, "num": 4} for u in range(0, 50, 4)]
    qs += [{"user": 999}, {}, {"item": 5}]
    for blacklist in (None, [], ["purchase", "view"]):
        algo.ap.blacklistEvents = blacklist
        want = algo.batch_predict(model, qs, history)
        got = algo.batch_predict(model, qs, dh)
        for q, w, g in zip(qs, want, got):
            assert g == w, (blacklist, q)
    assert any(s["score"] > 0 for r in want for s in r["itemScores"])


def test_batch_predict_dict_against_from_streams(gpu_session):
    """DeviceHistory.from_streams -- integer user ids, shuffled events, int64 times with ties and negative values, one type without times -- gives
    batch_predict the answers of the dict sorted by (time, position) on the host; users resolved by a dict and by their integer id."""
    algo, model = H.predict_stack(gpu_session, 3000, 400, 250)
    streams, history = H.make_stream_history(41, 120, 400, 250)
    H.check_from_streams(gpu_session, algo, model, 120, streams, history)
