"""urcco_dev_props_* on the MI355X: the cases of tests/test_sim_props.py (tests/props_cases.py) and one larger shape -- 2^20 + 77 property events over 2^16
items with a Zipf(1.2) item distribution (the hottest item of the largest stream takes more than 50 000 of its events), a third of them $unsets, 500 $deletes, two list properties and
one date, applied in three batches through properties.DeviceProperties and checked against the numpy form of tests/props_ref.py."""
import numpy as np
import pytest
import torch

import props_cases as PC
import props_ref as P

pytestmark = pytest.mark.gpu


def test_ties_and_revival(gpu_session):
    PC.tie_cases(gpu_session)


def test_batching_and_permutations(gpu_session):
    PC.batching_cases(gpu_session)


def test_time_and_item_domain(gpu_session):
    PC.domain_cases(gpu_session)


def test_rows_class_edges_and_capacity(gpu_session):
    PC.rows_cases(gpu_session)


def test_malformed_state_stays_inside_the_arrays(gpu_session):
    PC.malformed_state_cases(gpu_session)


def test_contention_on_one_item(gpu_session):
    PC.contention_case(gpu_session)


def test_bad_arguments(gpu_session):
    PC.bad_argument_cases(gpu_session)


class _Model:
    """what DeviceProperties reads of a model: the size of the primary's dictionary, dense integer ids"""

    def __init__(self, sess, n_items):
        self.sess, self.n_items = sess, n_items


def _csr_of_winners(n_items, n_cols, alive, pos, vp, vals):
    """the item x value matrix of the alive winners, in numpy: (row_ptr, col_idx, pair rows, pair cols)"""
    it = np.flatnonzero(alive)
    lo, ln = vp[pos[it]], vp[pos[it] + 1] - vp[pos[it]]
    rows = np.repeat(it, ln)
    at = np.repeat(lo - np.concatenate(([0], np.cumsum(ln)[:-1])), ln) + np.arange(int(ln.sum()))
    cols = vals[at].astype(np.int64)
    ok = (cols >= 0) & (cols < n_cols)
    rows, cols = rows[ok], cols[ok]
    key = np.unique(rows * n_cols + cols)
    rp = np.zeros(n_items + 1, np.int64)
    np.cumsum(np.bincount(key // n_cols, minlength=n_items), out=rp[1:])
    return rp, (key % n_cols).astype(np.int32), rows.astype(np.int32), cols.astype(np.int32)


def test_larger_shape(gpu_session):
    from universal_recommender_amd import ingest
    from universal_recommender_amd.properties import DeviceProperties
    sess = gpu_session
    rng = np.random.default_rng(47)
    n, n_items = (1 << 20) + 77, 1 << 16
    sizes = {"categories": (n - 2 * (n // 4), 900), "tags": (n // 4, 70_000), "expires": (n // 4, 0)}
    dp = DeviceProperties(sess, _Model(sess, n_items), ["expires"])
    dp.apply_streams({}, new_values={name: [f"v{j}" for j in range(c)] for name, (_, c) in sizes.items() if c})
    host = {}
    for name, (m, n_cols) in sizes.items():
        items = ((rng.zipf(1.2, m) - 1) % n_items).astype(np.int32)
        items[rng.integers(0, m, 200)] = np.array([-1, n_items, PC.I32_MIN, PC.I32_MAX], np.int32)[rng.integers(0, 4, 200)]
        times = (PC.T0 + rng.integers(0, 5000, m)).astype(np.int64)          # every hot item sees many equal times: the position decides
        times[rng.integers(0, m, 50)] = PC.I64_MIN
        kinds = (rng.random(m) < 1 / 3).astype(np.uint8)
        if n_cols:
            lens = np.where(kinds == P.SET, rng.integers(0, 5, m), 0)
            long = rng.choice(np.flatnonzero(kinds == P.SET), 3, replace=False)                    # a few long lists that win: the block classes
            lens[long], items[long], times[long] = [70, 5000, 4097], [1000, 1001, 1002], PC.T0 + 6000
            vp = np.zeros(m + 1, np.int64)
            np.cumsum(lens, out=vp[1:])
            vals = rng.integers(-1, n_cols + 1, int(vp[-1])).astype(np.int32)
            payload = (vp, vals)
        else:
            payload = rng.integers(-10**9, 10**13, m).astype(np.int64)
        host[name] = (items, times, kinds, payload)
    assert np.bincount(host["categories"][0][(host["categories"][0] >= 0) & (host["categories"][0] < n_items)]).max() > 50_000
    d_items, d_times = rng.integers(-1, n_items + 1, 500).astype(np.int32), (PC.T0 + rng.integers(0, 5000, 500)).astype(np.int64)
    d_items[:100] = np.arange(100)                                             # the hot items among them
    for lo, hi in ((0.0, 0.45), (0.45, 0.45), (0.45, 1.0)):                    # three batches, one of them empty
        batch = {}
        for name, (items, times, kinds, payload) in host.items():
            a, b = int(lo * items.size), int(hi * items.size)
            part = payload[a:b] if sizes[name][1] == 0 else (payload[0][a:b + 1] - payload[0][a], payload[1][payload[0][a]:payload[0][b]])
            batch[name] = (items[a:b], times[a:b], kinds[a:b], part)
        a, b = int(lo * 500), int(hi * 500)
        dp.apply_streams(batch, (d_items[a:b], d_times[a:b]))
    t_del = P.delete_np(n_items, d_items, d_times)
    assert np.array_equal(dp.t_del.cpu().numpy().view(np.uint64), t_del)
    want = {name: P.aggregate_np(n_items, items, times, kinds) for name, (items, times, kinds, _) in host.items()}
    for name, s in dp.streams.items():
        got = (s.t_set.cpu().numpy().view(np.uint64), s.pos_set.cpu().numpy().view(np.uint32), s.t_unset.cpu().numpy().view(np.uint64))
        for a, b, what in zip(got, want[name], ("t_set", "pos_set", "t_unset")):
            assert np.array_equal(a, b), (name, what)
    props, dates = dp.materialise()
    assert set(props) == {"categories", "tags"} and set(dates) == {"expires"}
    for name, p in props.items():
        t_set, pos_set, t_unset = want[name]
        alive = P.alive_np(t_set, t_unset, t_del)
        assert 1000 < alive.sum() < n_items
        vp, vals = host[name][3]
        w_rp, w_ci, pr, pc = _csr_of_winners(n_items, p.n_cols, alive, pos_set.astype(np.int64) - 1, vp, vals)
        assert np.array_equal(p.row_ptr.cpu().numpy(), w_rp) and np.array_equal(p.col_idx.cpu().numpy(), w_ci), name
        assert np.diff(w_rp).max() > 64
        m = ingest.csr_from_pairs(sess, torch.from_numpy(pr).to(sess.device), torch.from_numpy(pc).to(sess.device), n_items, p.n_cols)
        assert torch.equal(m.row_ptr, p.row_ptr) and torch.equal(m.col_idx[: m.nnz_bound], p.col_idx), name
        assert int(p.col_ptr[-1]) == w_ci.size and np.array_equal(np.diff(p.col_ptr.cpu().numpy()), np.bincount(w_ci, minlength=p.n_cols))
    t_set, pos_set, t_unset = want["expires"]
    alive = P.alive_np(t_set, t_unset, t_del)
    w_dates = np.where(alive, host["expires"][3][np.where(alive, pos_set.astype(np.int64) - 1, 0)], P.I64_MIN)
    assert np.array_equal(dates["expires"].cpu().numpy(), w_dates)
    mask = dp.item_mask().cpu().numpy()
    w_mask = P.exists_np([want[name][0] for name in dp.streams], t_del)
    assert np.array_equal(mask, w_mask) and 0 < (w_mask == 0).sum() < 500
