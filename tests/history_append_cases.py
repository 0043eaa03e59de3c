"""urcco_dev_history_append (decision D21 of DESIGN.md, include/urcco.h): the problems and checks that tests/test_sim_history_append.py and
tests/test_gpu_history_append.py share.  The contract, restated in numpy: the index after an append is an index of the concatenated stream whose
row_ptr is that of urcco_dev_history_index over the whole stream, and every user's segment is its old segment verbatim, then a permutation of
n_old + flatnonzero(new_users == u).

make_edge_problem is built from the copy kernel's own constants (HA_TILE entries per block, HA_LDS_USERS users staged in LDS; read from
csrc/cco_history.h): tiles inside one user, tiles over few users, a tile of one-event users (the most users a tile without empty ones touches, staged),
tiles over more users than the staging holds (they cross a run of empty users), runs of empty users at both ends."""
import copy
import os
import re
from dataclasses import dataclass

import numpy as np
import torch

import history_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constants():
    text = open(os.path.join(ROOT, "universal-recommender_amd", "csrc", "cco_history.h")).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", text).group(1)) for name in ("HA_TILE", "HA_LDS_USERS"))


HA_TILE, HA_LDS_USERS = kernel_constants()


def put(sess, a):
    """a numpy array in a tensor of exactly its size from the session's allocator (guarded under HIPSIM_GUARD)"""
    t = sess.empty(a.size, torch.from_numpy(a[:0].copy()).dtype)
    if a.size:
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def row_ptr_ref(users, n_users):
    """row_ptr of an index of `users` over n_users users: ids < 0 or >= n_users are nobody's"""
    ok = users[(users >= 0) & (users < n_users)]
    return np.concatenate([[0], np.cumsum(np.bincount(ok, minlength=n_users))]).astype(np.int64)


def check_append(old_rp, old_pos, n_old, new_users, n_users, rp, pos):
    """The contract for one append, all numpy.  old_rp None: no old index."""
    n_users_old = old_rp.size - 1 if old_rp is not None else 0
    old_rp = old_rp if old_rp is not None else np.zeros(1, np.int64)
    assert rp.size == n_users + 1 and rp[0] == 0
    valid = (new_users >= 0) & (new_users < n_users)
    add = np.concatenate([[0], np.cumsum(np.bincount(new_users[valid], minlength=n_users))])
    old_start = old_rp[np.minimum(np.arange(n_users + 1), n_users_old)]
    assert np.array_equal(rp, old_start + add), "row_ptr is not old row_ptr + the batch's prefix"
    old_cnt = np.diff(old_start)
    # the old segments verbatim: old entry e of user u sits at e + add[u]
    n_e = int(old_rp[-1])
    owner = np.repeat(np.arange(n_users_old), np.diff(old_rp))
    assert n_e == 0 or np.array_equal(pos[np.arange(n_e) + add[owner]], old_pos[:n_e]), "an old segment was not copied verbatim"
    # behind them a permutation of the batch's positions of that user
    tail = np.ones(int(rp[-1]), bool)
    tail[np.arange(n_e) + add[owner]] = False
    tail_owner = np.repeat(np.arange(n_users), np.diff(rp) - old_cnt)
    assert np.array_equal(np.repeat(np.arange(n_users), np.diff(rp))[tail], tail_owner), "the new positions are not behind the old segments"
    got = pos[: int(rp[-1])][tail]
    order = np.lexsort((got, tail_owner))
    want = n_old + np.flatnonzero(valid)
    want = want[np.argsort(new_users[valid], kind="stable")]
    assert np.array_equal(got[order], want), "a user's new positions are not n_old + flatnonzero(new_users == u)"


def append_chain(sess, users, cuts, n_users_seq, null_old=False):
    """history_index of users[:cuts[0]] over n_users_seq[0] users, then one history_append per further cut (the last one ends the stream), each
    checked against the contract.  null_old: cuts[0] must be 0, the first append gets no old index at all.  Returns the final (row_ptr, pos) tensors."""
    cuts = list(cuts) + [users.size]
    assert len(n_users_seq) == len(cuts)
    if null_old:
        assert cuts[0] == 0
        rp = pos = None
    else:
        rp, pos = sess.history_index(put(sess, users[: cuts[0]]), n_users_seq[0])
    for a, b, n_users in zip(cuts[:-1], cuts[1:], n_users_seq[1:]):
        new_rp, new_pos = sess.history_append(rp, pos, a, put(sess, users[a:b]), n_users)
        sess.synchronize()
        assert new_rp.numel() == n_users + 1 and new_pos.numel() == max(b, 1)          # exact sizes: a write past them faults under HIPSIM_GUARD
        check_append(rp.cpu().numpy() if rp is not None else None, pos.cpu().numpy() if pos is not None else None, a, users[a:b], n_users,
                     new_rp.cpu().numpy(), new_pos.cpu().numpy())
        rp, pos = new_rp, new_pos
    assert np.array_equal(rp.cpu().numpy(), row_ptr_ref(users, n_users_seq[-1]))
    return rp, pos


def index_cases(sess, p: H.Problem):
    """Case 1 of the tests: every stream of the problem split once, three times, at 0 (empty old index, and none) and at its end."""
    for s in p.streams:
        n, nu = s.users.size, p.n_users
        full_rp, _ = sess.history_index(put(sess, s.users), nu)
        sess.synchronize()
        full_rp = full_rp.cpu().numpy()
        for cuts, null_old in (([n * 2 // 3], False), ([n // 4, n // 2, n * 3 // 4], False), ([0], False), ([0], True), ([n], False)):
            rp, pos = append_chain(sess, s.users, cuts, [nu] * (len(cuts) + 1), null_old)
            rp, rows = H.csr_rows(rp, pos)
            assert np.array_equal(rp, full_rp)
            for u, r in enumerate(rows):
                assert np.array_equal(np.sort(r), np.flatnonzero(s.users == u))


# ---- the constructed problem of the copy kernel's edges -----------------------------------------------------------------------------------------
@dataclass
class EdgeProblem:
    old_users: np.ndarray    # int32: the old stream
    n_users_old: int
    new_users: np.ndarray    # int32: the batch
    n_users: int
    old_counts: np.ndarray   # events per user of the old stream
    named: dict              # user ids the asserts name


def make_edge_problem(seed=7):
    T, L = HA_TILE, HA_LDS_USERS
    rng = np.random.default_rng(seed)
    counts, named = [], {}

    def add(name, cs):
        named[name] = len(counts)
        counts.extend(int(c) for c in cs)

    add("empty_front", [0] * (L + 5))
    add("long", [3 * T + 17])                    # from entry 0: the tiles 0, 1, 2 lie inside it, tile 3 begins in it
    add("to_boundary", [T - 17])                 # ends at 4 T: the next user begins exactly on a tile boundary
    add("on_boundary", [T + 1])                  # ends at 5 T + 1: the next user begins one entry behind a tile boundary
    add("off_boundary", [5])
    add("small", [0, 1, 63, 64, 65])
    add("empty_middle", [0] * (L + 5))
    add("ones", [1] * (2 * T + 5))               # a whole tile of users with one event each, wherever it begins: T users, the most a tile without empty users touches
    add("threes", [3] * 600)                     # tiles over several hundred users: staged
    add("random", rng.integers(0, 31, 300))
    add("empty_back", [0] * (L + 5))
    counts = np.array(counts, np.int64)
    n_users_old = counts.size
    old_users = np.repeat(np.arange(n_users_old, dtype=np.int32), counts)
    old_users = np.concatenate([old_users, np.full(9, -1, np.int32)])
    old_users = old_users[rng.permutation(old_users.size)]
    n_users = n_users_old + 7
    quiet = np.zeros(n_users, bool)              # users that get nothing new
    quiet[[named["to_boundary"], named["small"] + 3]] = True
    quiet[named["threes"]:named["threes"] + 600:2] = True
    quiet[n_users - 1] = True
    loud = np.flatnonzero(~quiet)
    new_users = np.concatenate([rng.choice(loud, 2500), np.full(300, named["long"]), np.arange(n_users_old, n_users - 1), np.arange(n_users_old, n_users - 1),
                                rng.integers(named["empty_middle"], named["empty_middle"] + L + 5, 40), [named["empty_front"], named["empty_back"] + L + 4],
                                [-1, -1, -5, n_users, n_users + 3]]).astype(np.int32)
    new_users = new_users[rng.permutation(new_users.size)]
    return EdgeProblem(old_users, n_users_old, new_users, n_users, counts, named)


def assert_edge_cases(e: EdgeProblem):
    """From the problem alone: what make_edge_problem promises."""
    T, L = HA_TILE, HA_LDS_USERS
    assert e.old_users.size + e.new_users.size <= 50000
    rp = row_ptr_ref(e.old_users, e.n_users_old)
    cnt = np.diff(rp)
    assert np.array_equal(cnt, e.old_counts)
    n_e = int(rp[-1])
    assert n_e < e.old_users.size                                            # the old stream holds nobody's events: n_old is above the entries
    first_tile, last_tile = rp[:-1] // T, (rp[1:] - 1) // T
    assert ((cnt > 0) & (last_tile - first_tile >= 3)).any()                 # a segment over at least three tiles (it covers whole ones)
    starts = rp[:-1][cnt > 0]
    assert ((starts % T == 0) & (starts > 0)).any() and (starts % T == 1).any()   # a tile boundary on a user boundary, and one entry off
    runs = []                                                                # (first user, length) of the maximal runs of empty users
    u = 0
    while u < cnt.size:
        if cnt[u] == 0:
            v = u
            while v < cnt.size and cnt[v] == 0:
                v += 1
            runs.append((u, v - u))
            u = v
        else:
            u += 1
    long_runs = [(a, n) for a, n in runs if n > L]
    assert any(a == 0 for a, _ in long_runs) and any(a + n == cnt.size for a, n in long_runs) and any(a > 0 and a + n < cnt.size for a, n in long_runs)
    assert any(cnt[i:i + 5].tolist() == [0, 1, 63, 64, 65] for i in range(cnt.size - 5))
    # the users of every tile: one (a plain copy); several; a whole tile of one-event users (T users: staged in LDS, the staging holds at least T);
    # more than the staging holds -- which takes a run of empty users inside the tile
    owner = np.repeat(np.arange(cnt.size), cnt)
    tiles = [(int(owner[a]), int(owner[min(a + T, n_e) - 1])) for a in range(0, n_e, T)]
    spans = np.array([hi - lo + 1 for lo, hi in tiles])
    assert L >= T and (spans == 1).any() and ((spans > 1) & (spans < T)).any()
    assert any(hi - lo + 1 == T and (cnt[lo:hi + 1] == 1).all() for lo, hi in tiles)
    assert any(hi - lo + 1 > L for lo, hi in tiles) and all((cnt[lo:hi + 1] == 0).any() for lo, hi in tiles if hi - lo + 1 > L)
    nu = e.new_users
    assert ((nu >= e.n_users_old) & (nu < e.n_users)).any() and (nu == -1).any() and (nu < -1).any() and (nu == e.n_users).any() and (nu > e.n_users).any()
    new_cnt = np.bincount(nu[(nu >= 0) & (nu < e.n_users)], minlength=e.n_users)
    assert ((cnt > 0) & (new_cnt[:cnt.size] == 0)).any() and ((cnt > 0) & (new_cnt[:cnt.size] > 0)).any() and ((cnt == 0) & (new_cnt[:cnt.size] > 0)).any()
    assert new_cnt[e.n_users - 1] == 0                                       # the id space grows past the last user anybody names
    for a, n in long_runs:                                                   # the shift changes inside every long run of empty users
        assert new_cnt[a:a + n].any()


def edge_case(sess, e: EdgeProblem, pad=0):
    """The constructed problem through one append; pad > 0: that many sentinel entries behind both outputs, none of them written."""
    rp, pos = sess.history_index(put(sess, e.old_users), e.n_users_old)
    n_old, n_new = e.old_users.size, e.new_users.size
    out = None
    if pad:
        out = (sess.empty(e.n_users + 1 + pad, torch.int64), sess.empty(n_old + n_new + pad, torch.int32))
        out[0].fill_(H.SENTINEL)
        out[1].fill_(H.SENTINEL)
    new_rp, new_pos = sess.history_append(rp, pos, n_old, put(sess, e.new_users), e.n_users, out)
    sess.synchronize()
    check_append(rp.cpu().numpy(), pos.cpu().numpy(), n_old, e.new_users, e.n_users, new_rp.cpu().numpy(), new_pos.cpu().numpy())
    assert np.array_equal(new_rp.cpu().numpy(), row_ptr_ref(np.concatenate([e.old_users, e.new_users]), e.n_users))
    if pad:
        # behind the row starts, and behind the index entries (out_pos has room for n_old + n_new, the index holds fewer: nobody's events)
        assert (out[0][e.n_users + 1:] == H.SENTINEL).all() and (out[1][int(new_rp[-1]):] == H.SENTINEL).all()


# ---- rows over an appended index ----------------------------------------------------------------------------------------------------------------
ROW_CAPS = (5, 100)
TIME_SHIFT = 1000        # make_problem draws its times from 50 consecutive values: a shift of 1000 is older / newer than all of them


def make_rows_problem():
    """make_problem() with every stream cut at two thirds; the batch's times (streams 0 and 2; stream 1 has none) in three parts: as drawn (equal
    to old ones: ties across the cut), older than every old time, newer than every old time.  Returns (problem, cuts)."""
    p = H.make_problem()
    cuts = []
    for s in p.streams:
        n = s.users.size
        cut = n * 2 // 3
        cuts.append(cut)
        if s.times is not None:      # few newer ones: a window of 100 of a user with 4096 events then still reaches back into the old events
            s.times[cut + (n - cut) * 9 // 20:n - (n - cut) // 20] -= TIME_SHIFT
            s.times[n - (n - cut) // 20:] += TIME_SHIFT
    return p, cuts


def assert_rows_problem(p: H.Problem, cuts, by_user):
    """An event that arrived late with an old time stays outside a window that an earlier event is in; late events with new times are in"""
    assert p.streams[1].times is None and p.streams[0].times is not None
    s, cut = p.streams[0], cuts[0]
    old_t = s.times[:cut]
    new_t = s.times[cut:]
    assert (new_t < old_t.min()).any() and (new_t > old_t.max()).any() and np.isin(new_t, old_t).any()
    for cap in ROW_CAPS:
        late_old_time_out = late_in = False
        for ev in by_user[0]:
            if ev.size > cap:
                w, rest = ev[:cap], ev[cap:]
                late_old_time_out |= bool((w < cut).any() and ((rest >= cut) & (s.times[rest] < old_t.min())).any())
                late_in |= bool((w >= cut).any())
        assert late_old_time_out and late_in, cap


def rows_case(sess, p: H.Problem, cuts):
    """Case 3: term and exclusion rows over the appended index == over the from-scratch index == the restatement, caps 5 and 100"""
    scratch = H.DeviceProblem(sess, p)
    assert_rows_problem(p, cuts, scratch.by_user)
    appended = copy.copy(scratch)
    appended.ev = []
    for s, cut, (n_cols, _, _, items, times, cmap) in zip(p.streams, cuts, scratch.ev):
        rp, pos = append_chain(sess, s.users, [cut], [p.n_users, p.n_users])
        appended.ev.append((n_cols, rp, pos, items, times, cmap))
    for cap in ROW_CAPS:
        _, terms_a, excl_a = H.check(scratch, [cap] * 3)
        _, terms_b, excl_b = H.check(appended, [cap] * 3)
        for ra, rb in zip(terms_a + [excl_a], terms_b + [excl_b]):
            assert all(np.array_equal(x, y) for x, y in zip(ra, rb))


# ---- the handmade golden's model and queries (tests/golden/handmade.json), for DeviceHistory.append_dict ------------------------------------------
def handmade_stack(sess, cap=None):
    """(algorithm, device model, history user -> {event: [ids, oldest first]}, all items): the handmade fixture trained on the session, maxItemsPerUser
    = cap where given, and one more user the model never saw with more purchases than any cap here, an id no dictionary holds among them"""
    import json
    from universal_recommender_amd.data_source import DataSource, DataSourceParams
    from universal_recommender_amd.preparator import Preparator
    from universal_recommender_amd.recommend import DeviceModel
    from universal_recommender_amd.ur_algorithm import URAlgorithm, URAlgorithmParams
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "handmade.json")))
    history, items = {}, []
    for u, e, i in doc["events"]:
        history.setdefault(u, {}).setdefault(e, []).append(i)
        if i not in items:
            items.append(i)
    lines = [",".join(e) for e in doc["events"]] + [f"{i},$set,{p}" for i, p in doc["sets"]]
    engine = {"datasource": {"params": doc["datasource_params"]}, "algorithms": [{"name": "ur", "params": doc["algorithm_params"]}]}
    td = DataSource(DataSourceParams.from_engine_json(engine)).readTraining(lines)
    ap = URAlgorithmParams.from_engine_json(engine)
    ap.seed = 1
    algo = URAlgorithm(ap, device=0, library=sess.lib)
    model = DeviceModel.from_indicators(sess, algo.train(Preparator().prepare(td)).coocurrenceMatrices, properties={})
    if cap is not None:
        for ind in ap.indicators:
            ind.maxItemsPerUser = cap
    purchases = [i for _, e, i in doc["events"] if e == "purchase"]
    history["heavy"] = {"purchase": purchases[:3] + ["no such item"] + [purchases[k % 2] for k in range(40)], "view": [i for _, e, i in doc["events"] if e == "view"][:7] + ["nothing"]}
    return algo, model, history, items


def handmade_queries(history, items):
    """user, user + item and bias queries over every user of the history and one nobody knows"""
    users = list(history) + ["nobody"]
    qs = [{"user": u} for u in users] + [{"user": u, "item": items[k % len(items)]} for k, u in enumerate(users)]
    qs += [{"user": u, "userBias": -1.0} for u in users[:4] + ["heavy", "nobody"]]
    qs += [{"user": u, "userBias": 2.5, "blacklistItems": items[k:k + 2]} for k, u in enumerate(users)]
    qs += [{"user": u, "eventNames": ["view", "purchase"]} for u in users[:3] + ["heavy"]]
    qs += [{}, {"item": items[0]}, {"itemSet": items[:2]}]
    return qs
