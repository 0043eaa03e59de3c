"""urcco_dev_history_append on the MI355X: the cases of tests/test_sim_history_append.py (tests/history_append_cases.py), one larger shape -- an old
index of 2^22 events over 2^18 users with a Zipf user distribution, a batch of 2^12 -- and DeviceHistory.append_dict against from_dict of the whole
history through batch_predict.  Every device step is one library call."""
import numpy as np
import pytest
import torch

import history_append_cases as A
import history_ref as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def edge():
    return A.make_edge_problem()


def test_index_after_appends(gpu_session):
    A.index_cases(gpu_session, H.make_problem())


def test_copy_kernel_edges(gpu_session, edge):
    A.assert_edge_cases(edge)
    A.edge_case(gpu_session, edge)


def test_nothing_written_behind_the_outputs(gpu_session, edge):
    A.edge_case(gpu_session, edge, pad=256)


def test_rows_over_an_appended_index(gpu_session):
    p, cuts = A.make_rows_problem()
    A.rows_case(gpu_session, p, cuts)


def test_larger_shape(gpu_session):
    """2^22 old events over 2^18 users, Zipf: one user owns about a fifth of them, most own none or one; 2^12 new events of the same distribution,
    some for ids beyond the old space.  row_ptr and the sorted segments against numpy; the old segments verbatim."""
    s = gpu_session
    rng = np.random.default_rng(29)
    n_old, n_new, n_users_old = 1 << 22, 1 << 12, 1 << 18
    n_users = n_users_old + 100
    old_users = ((rng.zipf(1.3, n_old) - 1) % n_users_old).astype(np.int32)
    new_users = ((rng.zipf(1.3, n_new) - 1) % n_users).astype(np.int32)
    new_users[:64] = rng.integers(n_users_old, n_users, 64)
    new_users[64:72] = -1
    cnt = np.bincount(old_users, minlength=n_users_old)
    assert cnt.max() > 500_000 and np.count_nonzero(cnt == 0) > n_users_old // 4
    rp, pos = s.history_index(A.put(s, old_users), n_users_old)
    new_rp, new_pos = s.history_append(rp, pos, n_old, A.put(s, new_users), n_users)
    s.synchronize()
    h_rp, h_pos = new_rp.cpu().numpy(), new_pos.cpu().numpy()
    A.check_append(rp.cpu().numpy(), pos.cpu().numpy(), n_old, new_users, n_users, h_rp, h_pos)
    users = np.concatenate([old_users, new_users])
    assert np.array_equal(h_rp, A.row_ptr_ref(users, n_users))
    owner = np.repeat(np.arange(n_users), np.diff(h_rp))
    want = np.flatnonzero(users >= 0)
    want = want[np.argsort(users[want], kind="stable")]                  # by user, positions ascending
    assert np.array_equal(h_pos[: h_rp[-1]][np.lexsort((h_pos[: h_rp[-1]], owner))], want)


def test_append_dict_against_from_dict(gpu_session):
    """A device-built model over integer ids; half of every user's history loaded, the rest appended, the last ten users unseen by the first load"""
    from universal_recommender_amd.history import DeviceHistory
    algo, model = H.predict_stack(gpu_session, 3000, 400, 250)
    rng = np.random.default_rng(31)
    history = {u: {"purchase": rng.integers(0, 420, rng.integers(0, 150)).tolist(), "view": rng.integers(0, 250, rng.integers(0, 150)).tolist()} for u in range(200)}
    first = {u: {ev: ids[: len(ids) // 2] for ev, ids in evs.items()} for u, evs in history.items() if u < 190}
    rest = {u: {ev: ids[len(ids) // 2:] if u < 190 else ids for ev, ids in evs.items()} for u, evs in history.items()}
    dh = DeviceHistory.from_dict(gpu_session, model, first).append_dict(model, rest)
    whole = DeviceHistory.from_dict(gpu_session, model, history)
    assert dh.n_users == whole.n_users == 200
    qs = [{"user": u} for u in range(0, 200, 3)] + [{"user": u, "item": int(u * 2)} for u in range(1, 200, 7)] + [{"user": u, "userBias": -1.0, "num": 5} for u in range(2, 60, 5)]
    qs += [{"user": 999}, {}, {"item": 5}]
    for weights in (None, "idf"):
        for blacklist in (None, ["purchase", "view"]):
            algo.ap.blacklistEvents = blacklist
            want = algo.batch_predict(model, qs, whole, term_weights=weights)
            assert algo.batch_predict(model, qs, dh, term_weights=weights) == want
    algo.ap.blacklistEvents = None
    assert any(s["score"] > 0 for r in want for s in r["itemScores"])
    assert all(torch.equal(a, b) for a, b in zip(algo.user_recommendations(model, dh), algo.user_recommendations(model, whole)))
