"""A history by key (decision D26: DeviceHistory.from_key_streams / append_keys / user_indices, DeviceModel.key_dictionary), shared by
test_history_keys_predict.py (the simulator session) and test_gpu_history_keys.py: the handmade golden's model (tests/golden/handmade.json) and its
users' events, fed as streams of 64-bit keys in four batches, against DeviceHistory.from_streams over dense ids from a host dict walked in the same order.

The batches: user number j of the history first appears in batch j % 4 and has its events spread over the batches from there on, so every batch after
the first holds users the dictionary knows and users it does not, and the last one users nobody saw before.  The "heavy" user of
history_append_cases.handmade_stack carries two item ids no dictionary holds."""
import numpy as np
import torch

import history_append_cases as A

EVENTS = ["purchase", "view", "category-pref"]
N_BATCHES = 4


def batches_of(history):
    """[{event: [(user, item), ...]} per batch], every user's list of an event in its own order across the batches"""
    out = [{ev: [] for ev in EVENTS} for _ in range(N_BATCHES)]
    for j, (u, evs) in enumerate(history.items()):
        first = j % N_BATCHES
        parts = N_BATCHES - first
        for ev in EVENTS:
            ids = evs.get(ev, [])
            cuts = [len(ids) * k // parts for k in range(parts + 1)]
            for k in range(parts):
                out[first + k][ev] += [(u, i) for i in ids[cuts[k]:cuts[k + 1]]]
    return out


def keyed(sess, batch, model=None, dense=(), check=False):
    """A batch as from_key_streams takes it: user keys, item keys (dense int32 column ids for the events in `dense`), no times[, user check keys]"""
    from universal_recommender_amd.preparator import CHECK_SEED, hash_keys
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(sess.device)
    out = {}
    for ev, pairs in batch.items():
        users, items = [u for u, _ in pairs], [i for _, i in pairs]
        if ev in dense:
            ids = [model.column_index(model.by_name[ev], i) for i in items]
            cols = dev(np.asarray([-1 if i is None else i for i in ids], np.int32))
        else:
            cols = dev(hash_keys(items, library=sess.lib))
        out[ev] = (dev(hash_keys(users, library=sess.lib)), cols, None) + ((dev(hash_keys(users, CHECK_SEED, sess.lib)),) if check else ())
    return out


def dense_reference(sess, model, batches):
    """(host dict user -> id walked batch by batch, event by event; DeviceHistory.from_streams over the batches laid end to end)"""
    from universal_recommender_amd.history import DeviceHistory
    user_ids, streams = {}, {ev: ([], []) for ev in EVENTS}
    for batch in batches:
        for ev in EVENTS:
            for u, i in batch[ev]:
                c = model.column_index(model.by_name[ev], i)
                streams[ev][0].append(user_ids.setdefault(u, len(user_ids)))
                streams[ev][1].append(-1 if c is None else c)
    dev = {ev: (torch.tensor(us, dtype=torch.int32).to(sess.device), torch.tensor(cs, dtype=torch.int32).to(sess.device), None) for ev, (us, cs) in streams.items()}
    return user_ids, DeviceHistory.from_streams(sess, model, dev, user_ids)


def same_streams(dh, ref):
    assert dh.n_users == ref.n_users and set(dh.types) == set(ref.types)
    for ev, st in dh.types.items():
        w = ref.types[ev]
        assert st.n_events == w.n_events and st.n_cols == w.n_cols and (st.col_map is None) == (w.col_map is None), ev
        assert torch.equal(st.items[: st.n_events], w.items[: w.n_events]) and torch.equal(st.idx_row_ptr, w.idx_row_ptr), ev
        rp = st.idx_row_ptr.cpu().tolist()      # a user's segment of the index is a set: its order is the hardware's (the rows are cut by time and position)
        a, b = st.idx_pos[: st.n_events].cpu().tolist(), w.idx_pos[: w.n_events].cpu().tolist()
        assert all(sorted(a[s:e]) == sorted(b[s:e]) for s, e in zip(rp, rp[1:])), ev


def history_rows_of(sess, model, dh, q_users):
    """DeviceSession.history_rows over the three event types for the dense query users: every row as host lists"""
    specs = [(dh.types[ev].n_cols, 3, ev == "purchase", dh.types[ev].idx_row_ptr, dh.types[ev].idx_pos, dh.types[ev].items, dh.types[ev].times, dh.types[ev].col_map)
             for ev in EVENTS]
    q = torch.tensor(q_users, dtype=torch.int32).to(sess.device)
    rows, excl, _ = sess.history_rows(q, dh.n_users, specs, model.n_items)
    flat = []
    for rp, ci in list(rows) + [excl]:
        rp = rp.cpu().tolist()
        flat.append((rp, ci.cpu().tolist()[: rp[-1]]))
    return flat


def case_keyed_history(sess):
    """from_key_streams + three append_keys against from_streams over the host dict: n_users, the streams and their indexes, history_rows, batch_predict
    with users named by string (an unknown one and one first seen in the last batch among them), trim(drop_users=[strings])."""
    from universal_recommender_amd.history import DeviceHistory
    algo, model, history, items = A.handmade_stack(sess, 3)
    batches = batches_of(history)
    users = list(history)
    assert len(users) >= 5 and "heavy" in users and all(any(b[ev] for ev in EVENTS) for b in batches)
    last = users[N_BATCHES - 1]                                          # first seen in the last batch
    assert not any(u == last for b in batches[:-1] for ev in EVENTS for u, _ in b[ev])
    assert any(model.column_index(model.by_name[ev], i) is None for b in batches for ev in EVENTS for _, i in b[ev]), "an item key outside the column dictionary"
    user_ids, ref = dense_reference(sess, model, batches)
    for dense in ((), ("view",)):                                        # every item by key; the views as dense int32 ids
        dh = DeviceHistory.from_key_streams(sess, model, keyed(sess, batches[0], model, dense))
        assert dh.user_ids is None and dh.user_dict is not None and dh.user_index(last) == -1
        seen = dh.n_users
        for b in batches[1:]:
            assert dh.append_keys(keyed(sess, b, model, dense)) is dh
            assert dh.n_users == dh.user_dict.n_ids > seen               # every batch brings new users
            seen = dh.n_users
        same_streams(dh, ref)
        asked = users + ["nobody", None]
        assert dh.user_indices(asked) == [user_ids[u] for u in users] + [-1, -1] == ref.user_indices(asked)
        assert dh.user_index(last) == user_ids[last] and dh.user_index("nobody") == -1
        q_users = dh.user_indices(asked)
        assert history_rows_of(sess, model, dh, q_users) == history_rows_of(sess, model, ref, q_users)
        qs = A.handmade_queries(history, items)
        assert any(q.get("user") == last for q in qs) and any(q.get("user") == "nobody" for q in qs)
        for weights in (None, "idf"):
            want = algo.batch_predict(model, qs, ref, term_weights=weights)
            assert algo.batch_predict(model, qs, dh, term_weights=weights) == want == algo.batch_predict(model, qs, history, term_weights=weights), weights
            assert any(s["score"] > 0 for r in want for s in r["itemScores"])
        named = [users[1], last, "nobody"]
        assert all(torch.equal(a, b) for a, b in zip(algo.user_recommendations(model, dh, named), algo.user_recommendations(model, ref, named)))
    # the event store's $delete of users, by string
    drop = ["heavy", last, "nobody"]
    dh.trim(drop_users=drop)
    _, ref2 = dense_reference(sess, model, batches)
    ref2.trim(drop_users=drop)
    same_streams(dh, ref2)
    assert dh.last_trim == ref2.last_trim and any(a != b for a, b in dh.last_trim.values())
    assert algo.batch_predict(model, qs, dh) == algo.batch_predict(model, qs, ref2) != want
    dh.append_keys(keyed(sess, batches[1], model))                       # and the history works on: the dropped users keep their ids
    ref2.append({ev: (torch.tensor([user_ids[u] for u, _ in batches[1][ev]], dtype=torch.int32).to(sess.device),
                      torch.tensor([-1 if (c := model.column_index(model.by_name[ev], i)) is None else c for _, i in batches[1][ev]], dtype=torch.int32).to(sess.device),
                      None) for ev in EVENTS})
    same_streams(dh, ref2)


def case_evaluate_over_a_shared_dictionary(sess):
    """The training history from the first three batches, the held-out history from the last one over the SAME dictionary object: the last batch brings
    users the training history never saw, append_keys({}) levels it; the report equals the one over dense ids."""
    from universal_recommender_amd.history import DeviceHistory
    import pytest
    algo, model, history, _ = A.handmade_stack(sess, 3)
    batches = batches_of(history)
    train = DeviceHistory.from_key_streams(sess, model, keyed(sess, batches[0]))
    for b in batches[1:-1]:
        train.append_keys(keyed(sess, b))
    test = DeviceHistory.from_key_streams(sess, model, keyed(sess, batches[-1]), user_dict=train.user_dict)
    assert test.user_dict is train.user_dict and test.n_users > train.n_users
    with pytest.raises(ValueError):
        algo.evaluate(model, train, test, ks=(1, 3), num=5)              # not level yet
    train.append_keys({})
    assert train.n_users == test.n_users
    other = DeviceHistory.from_key_streams(sess, model, keyed(sess, {ev: [p for b in batches for p in b[ev]] for ev in EVENTS}))
    assert other.n_users == test.n_users
    with pytest.raises(ValueError):
        algo.evaluate(model, train, other, ks=(1, 3), num=5)             # as many users, another dictionary
    user_ids, _ = dense_reference(sess, model, batches)
    n = len(user_ids)

    def dense(bs):
        out = {}
        for ev in EVENTS:
            pairs = [p for b in bs for p in b[ev]]
            cols = [model.column_index(model.by_name[ev], i) for _, i in pairs]
            out[ev] = (torch.tensor([user_ids[u] for u, _ in pairs], dtype=torch.int32).to(sess.device),
                       torch.tensor([-1 if c is None else c for c in cols], dtype=torch.int32).to(sess.device), None)
        return out
    want = algo.evaluate(model, DeviceHistory.from_streams(sess, model, dense(batches[:-1]), n_users=n),
                         DeviceHistory.from_streams(sess, model, dense(batches[-1:]), n_users=n), ks=(1, 3), num=5)
    got = algo.evaluate(model, train, test, ks=(1, 3), num=5)
    assert want["evaluated"] > 0
    assert {k: v for k, v in got.items() if k != "per_user"} == {k: v for k, v in want.items() if k != "per_user"}
    assert all(torch.equal(got["per_user"][k], want["per_user"][k]) for k in ("hits", "ap", "ndcg"))


def case_column_dictionaries_are_the_identity(sess):
    """model.key_dictionary(event): first-appearance ids over distinct strings in id order are those ids; a key outside the catalogue gives -1; an event name
    outside the model gets the primary's item dictionary; built once."""
    from universal_recommender_amd import ingest
    from universal_recommender_amd.preparator import hash_keys
    _, model, _, _ = A.handmade_stack(sess)
    for ev in EVENTS + ["an event outside the model"]:
        c = model.by_name.get(ev)
        names = c.column_ids if c is not None else model.item_ids
        d = model.key_dictionary(ev)
        assert d is model.key_dictionary(ev) and d.n_ids == len(names) > 0
        keys = torch.from_numpy(hash_keys(names.keys + ["no such item", ""], library=sess.lib)).to(sess.device)
        assert ingest.dictionary_lookup(sess, d, keys).cpu().tolist() == list(range(len(names))) + [-1, -1]
        assert [names.get(k) for k in names.keys] == list(range(len(names)))


def case_check_keys_and_refusals(sess):
    """check=True: the streams carry the users' check keys, a planted second string behind a user's key raises HashCollision; what append_keys refuses
    leaves the history and its dictionary as they were."""
    import pytest
    from universal_recommender_amd import ingest
    from universal_recommender_amd.history import DeviceHistory
    _, model, history, _ = A.handmade_stack(sess, 3)
    batches = batches_of(history)
    dh = DeviceHistory.from_key_streams(sess, model, keyed(sess, batches[0], check=True), check=True)
    dh.append_keys(keyed(sess, batches[1], check=True))
    n_users, n_events = dh.n_users, {ev: st.n_events for ev, st in dh.types.items()}
    good = keyed(sess, batches[2], check=True)
    k, i, t, c = good["purchase"]
    bad = [{"purchase": (k, i, t)}, {"purchase": (k.to(torch.int32), i, t, c)}, {"purchase": (k, i[:-1], t, c)}, {"purchase": (k, i.to(torch.float32), t, c)},
           {"purchase": (k, i, t, c[:-1])}, {"purchase": (k, i, torch.zeros(k.numel(), dtype=torch.int64), c)},        # times for a stream that has none
           {"view": good["view"], "purchase": (k, i, t, c[:-1])}]                                                     # the first stream is fine, the second is not
    for streams in bad:
        with pytest.raises(ValueError):
            dh.append_keys(streams)
        assert dh.n_users == dh.user_dict.n_ids == n_users and {ev: st.n_events for ev, st in dh.types.items()} == n_events
    planted = c.clone()
    planted[next(p for p, (u, _) in enumerate(batches[2]["purchase"]) if dh.user_index(u) >= 0)] ^= 0x10      # a second string behind the key of a user the dictionary knows
    with pytest.raises(ingest.HashCollision):
        dh.append_keys({"purchase": (k, i, t, planted)})
    with pytest.raises(ValueError):
        DeviceHistory.from_streams(sess, model, {}, n_users=3).append_keys(good)      # not a keyed history
