"""The growable device dictionary (csrc/cco_dictionary.h: dx_reserved / dx_insert / dx_firsts / dx_assign / dx_ids / dx_rehash; include/urcco.h
urcco_dev_dictionary_extend) on CONSTRUCTED keys, shared by test_sim_dictionary_extend.py and test_gpu_dictionary_extend.py.  The keys come from
dictionary_cases (mix / unmix / keys_at / capacity), so a case decides which slot each key calls home -- in the table before a rehash and in the one after.

Every comparison is exact and is made two ways (`run`):
  * against a Python dict walked in stream order -- after EVERY batch: n_ids, the ids of the batch's positions, new_pos;
  * against ONE dictionary_build over the start stream and all batches laid end to end: the same n_ids, the same lookup answers for every key seen and
    for the queries, and first_pos == the build's own first positions followed by batch offset + new_pos.
`repeat` (the hardware driver): the whole case runs that many times; every run equals the one restatement, hence every other run."""
import ctypes as C

import numpy as np
import pytest
import torch

import dictionary_cases as D
from universal_recommender_amd import _lib, ingest

INT32_MAX = 2 ** 31 - 1


def walk_batches(start, batches, selects):
    """The dict: (ids of the start stream, [(ids per position, new_pos, n_ids) per batch], the dict itself)."""
    ids = {}
    for k in start:
        ids.setdefault(k, len(ids))
    out = []
    for keys, sel in zip(batches, selects):
        new_pos, got = [], []
        for p, k in enumerate(keys):
            if sel is not None and sel[p] < 0:
                got.append(-1)
                continue
            if k not in ids:
                ids[k] = len(ids)
                new_pos.append(p)
            got.append(ids[k])
        out.append((got, new_pos, len(ids)))
    return out, ids


def run(sess, start, batches, selects=None, queries=(), repeat=1, checked=True):
    """build(start), extend(batch) for every batch: both comparisons of the module's head.  Returns the dict key -> id."""
    start = [int(k) for k in start]
    batches = [[int(k) for k in b] for b in batches]
    selects = list(selects) if selects is not None else [None] * len(batches)
    want, ids = walk_batches(start, batches, selects)
    d_start, d_batches, d_selects = D.dev_u64(sess, start), [D.dev_u64(sess, b) for b in batches], [D.dev_i32(sess, s) for s in selects]
    whole = start + [k for b in batches for k in b]
    whole_sel = None
    if any(s is not None for s in selects):
        whole_sel = [0] * len(start) + [v for b, s in zip(batches, selects) for v in (s if s is not None else [0] * len(b))]
    every = [k for k in dict.fromkeys(whole + list(queries)) if k != D.RESERVED] + ([D.RESERVED] if D.RESERVED in whole else [])
    d_every = D.dev_u64(sess, every)
    want_every = np.asarray([ids.get(k, -1) for k in every], np.int32)
    for r in range(repeat):
        d = ingest.dictionary_build(sess, d_start)
        one = ingest.dictionary_build(sess, D.dev_u64(sess, whole), D.dev_i32(sess, whole_sel))
        try:
            firsts, off = [d.first_pos.cpu().numpy()], len(start)
            for b, (dk, ds, (w_ids, w_new, w_n)) in enumerate(zip(d_batches, d_selects, want)):
                got_ids, got_new = d.extend(dk, ds)
                assert d.n_ids == w_n, (r, b, d.n_ids, w_n)
                assert int(got_ids.numel()) == len(w_ids) and D.same(got_ids, np.asarray(w_ids, np.int32)), (r, b)
                assert int(got_new.numel()) == len(w_new) and D.same(got_new, np.asarray(w_new, np.int64)), (r, b)
                firsts.append(got_new.cpu().numpy() + off)
                off += len(batches[b])
            assert D.same(ingest.dictionary_lookup(sess, d, d_every), want_every), r
            if checked:
                assert one.n_ids == d.n_ids, (r, one.n_ids, d.n_ids)
                assert D.same(ingest.dictionary_lookup(sess, one, d_every), want_every), r
                assert D.same(one.first_pos, np.concatenate(firsts)), r
        finally:
            d.close()
            one.close()
    return ids


def split(stream, cuts):
    """The stream cut at the positions `cuts` (ascending; equal neighbours give an empty batch)."""
    edges = [0] + list(cuts) + [len(stream)]
    return [stream[a:b] for a, b in zip(edges, edges[1:])]


def ordinary(first, count):
    """`count` distinct keys without a chosen home"""
    return [D.unmix(0x7700000 + first + i) for i in range(count)]


# ---- 1. batching ----------------------------------------------------------------------------------------------------------------------------------------
def batching_stream(seed=21, n=5000, distinct=1400):
    rng = np.random.default_rng(seed)
    pool = ordinary(0, distinct)
    return [pool[int(i)] for i in np.minimum(rng.zipf(1.3, n) - 1, rng.integers(0, distinct, n))]


def case_batching(sess, n_batches, repeat=1):
    stream = batching_stream()
    absent = ordinary(5000, 40)
    cuts = {1: [], 2: [1777], 7: [0, 300, 300, 2047, 2048, 4999]}[n_batches]       # 7: an empty first batch, an empty one in the middle, a batch of one key
    run(sess, [], split(stream, cuts), None, absent, repeat)                        # an empty table to start from
    run(sess, stream[:900], split(stream[900:], [c for c in cuts if c <= 4100]), None, absent, repeat)
    sel = D.mask_third(np.random.default_rng(22), stream)
    run(sess, [], split(stream, cuts), split(sel, cuts), absent, repeat)


# ---- 2. growth ------------------------------------------------------------------------------------------------------------------------------------------
def case_growth(sess, repeat=1):
    start = ordinary(0, 500)
    assert D.capacity(500) == 1024 and D.capacity(500 + 12) == 1024 and D.capacity(500 + 13) == 2048
    run(sess, start, [ordinary(900, 12)], None, ordinary(2000, 20), repeat)                       # 512 ids could be held: no rehash
    ids = run(sess, start, [start[100:113]], None, ordinary(2000, 20), repeat)                    # n_ids + n = 513: rehash to 2048 -- and all 13 are old keys
    assert len(ids) == 500
    run(sess, start, [start[100:113], ordinary(900, 12)], None, ordinary(2000, 20), repeat)       # the grown table takes new keys
    seven = [ordinary(10_000 + 300 * b, 300) + ordinary(10_000, 40) for b in range(7)]            # 1024 -> 2048 (batch 2) -> 4096 (batch 4) -> 8192 (batch 7)
    ids = run(sess, [], seven, None, ordinary(2000, 20), repeat)
    assert len(ids) == 2100 and D.capacity(300 + 340) == 2048 and D.capacity(900 + 340) == 4096


# ---- 3. probe chains -------------------------------------------------------------------------------------------------------------------------------------
def case_chain_wraps_then_rehash(sess, repeat=1):
    """300 keys of home slot 1023 of a table of 1024: the chain runs 1023, 0, 1, ..., 298.  A batch of all of them (old keys) and 250 new keys of the same
    home slot needs 2048 slots: after the rehash the keys call 1023 or 2047 home -- both chains are walked, the second one wraps again."""
    cap = D.MIN_CAPACITY
    ks, stream = D.chain_stream(cap - 1)
    fresh = D.keys_at(cap - 1, cap, 250, skip=len(ks) + 100)
    assert {D.home(k, 2 * cap) for k in ks + fresh} == {cap - 1, 2 * cap - 1}
    absent = D.keys_at(cap - 1, cap, 30, skip=1000) + D.keys_at(0, 2 * cap, 4) + D.keys_at(2 * cap - 1, 2 * cap, 4, skip=2000)
    rng = np.random.default_rng(31)
    batch = ks + fresh + fresh[:50]
    batch = [batch[i] for i in rng.permutation(len(batch))]
    assert D.capacity(len(ks) + len(batch)) == 2 * cap
    run(sess, stream, [batch], None, absent, repeat)
    run(sess, stream, [fresh[:100], batch], None, absent, repeat)       # no rehash (400 ids could be held), then the rehash: the wrapping chain grows first


def case_new_keys_in_old_chains(sess, repeat=1):
    cap = D.MIN_CAPACITY
    old = D.keys_at(50, cap, 100)                                        # slots 50 .. 149
    behind = D.keys_at(201, cap, 2)                                      # slots 201, 202
    start = old + behind + old[::3]
    new_in_chain = [k for s in (60, 100, 149, 150) for k in D.keys_at(s, cap, 3, skip=500)] + D.keys_at(50, cap, 20, skip=500)
    # an old key (201, 202) sits behind the slot (200) that a new key claims in this call: the other new keys of home 200 walk over both to 203, 204
    claim = D.keys_at(200, cap, 3, skip=500)
    batch = new_in_chain[:8] + behind + claim + old[:10] + new_in_chain[8:] + claim[::-1] + behind[::-1]
    assert D.capacity(len(set(start)) + len(batch)) == cap               # no rehash: the chains are the build's
    absent = D.keys_at(50, cap, 10, skip=900) + D.keys_at(200, cap, 4, skip=900) + D.keys_at(203, cap, 2)
    run(sess, start, [batch], None, absent, repeat)
    run(sess, start, [claim[:1], batch], None, absent, repeat)


# ---- 4. contention ----------------------------------------------------------------------------------------------------------------------------------------
def case_one_wave_one_slot(sess, base, repeat=1):
    """Batch positions base .. base + 63: 64 distinct NEW keys of one empty home slot; base + 64 .. base + 127: the same keys in reverse order."""
    start = [0x1000 + i for i in range(16)]
    n = base + 128
    cap = D.capacity(len(start) + n)
    ks = D.keys_at(5, cap, 64)
    batch = [start[i % 16] for i in range(base)] + ks + ks[::-1]
    ids = run(sess, start, [batch], None, (), repeat)
    assert [ids[k] for k in ks] == list(range(16, 80))                   # ids in position order, whoever won the slot
    sel = [0] * n
    for p in range(base, base + 64):
        sel[p] = -1                                                      # the forward block masked: the reversed block holds the firsts
    ids = run(sess, start, [batch], [sel], (), repeat)
    assert [ids[k] for k in ks[::-1]] == list(range(16, 80))


def case_hot_key(sess, times=100_000, repeat=1):
    start = ordinary(0, 50)
    rng = np.random.default_rng(41)
    for hot, grows in ((D.unmix(0xABCDEF), 1), (start[7], 0)):          # one NEW key / one OLD key `times` times, a few other keys in between
        batch = np.full(times + 200, hot, dtype=np.uint64)
        where = rng.choice(times + 200, 200, replace=False)
        batch[where] = np.asarray(ordinary(100, 20) * 10, dtype=np.uint64)
        ids = run(sess, start, [batch.tolist()], None, (), repeat)
        assert len(ids) == 50 + 20 + grows


# ---- 5. first appearances on the edges of the scan's tiles -----------------------------------------------------------------------------------------------
def case_tile_edges(sess, repeat=1):
    n = 3 * D.SCAN_TILE + 5
    firsts = [0, D.SCAN_TILE - 1, D.SCAN_TILE, D.SCAN_TILE + 1, n - 1]
    start = ordinary(0, 30)
    fresh = ordinary(100, len(firsts))
    rng = np.random.default_rng(5)
    batch, seen = [], list(start)
    for p in range(n):
        if p in firsts:
            seen.append(fresh[firsts.index(p)])
            batch.append(seen[-1])
        else:
            batch.append(seen[int(rng.integers(len(seen)))])
    want, _ = walk_batches(start, [batch], [None])
    assert want[0][1] == firsts
    run(sess, start, [batch], None, (), repeat)
    run(sess, [], [batch], None, (), repeat)


# ---- 6. select ---------------------------------------------------------------------------------------------------------------------------------------------
def case_select(sess, repeat=1):
    start = ordinary(0, 10)
    a, b, c = ordinary(100, 3)
    # position 1: the reserved key, masked -- accepted.  a: masked at 2, its first is position 5.  b: masked at 3 and 6, no id in this batch; its first is
    # position 1 of the NEXT batch.  c: masked everywhere, never an id.
    batch1 = [start[0], D.RESERVED, a, b, c, a, b, start[1], a]
    sel1 = [0, -1, -1, -2, -1, 5, -1, 0, 7]
    batch2 = [c, b, D.RESERVED, b, a]
    sel2 = [-1, 0, -3, 0, 0]
    ids = run(sess, start, [batch1, batch2], [sel1, sel2], [c], repeat)
    assert ids[a] == 10 and ids[b] == 11 and c not in ids and D.RESERVED not in ids
    want, _ = walk_batches(start, [batch1, batch2], [sel1, sel2])
    assert want[0][1] == [5] and want[1][1] == [1]


# ---- 7. extreme keys -----------------------------------------------------------------------------------------------------------------------------------------
def case_extreme_keys(sess, repeat=1):
    rng = np.random.default_rng(8)
    near = [2, (1 << 63) - 1, (1 << 63) + 1, (1 << 64) - 3]
    mixed = [D.EXTREME[int(i)] for i in rng.integers(0, 4, 200)]
    run(sess, [], [D.EXTREME], None, near, repeat)                                     # all four new
    run(sess, D.EXTREME[:2], [mixed, D.EXTREME[::-1]], None, near, repeat)             # two old, two new, then all old
    run(sess, ordinary(0, 5), [mixed[:100], near, mixed[100:]], None, (), repeat)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def extend_status(sess, d, n, keys, select, ids, new_pos, n_ids="out", session="own", table="own"):
    """urcco_dev_dictionary_extend called directly: (status, message, *n_ids)."""
    out = C.c_int64(-7)
    st = sess.lib.urcco_dev_dictionary_extend(sess.handle if session == "own" else None, d.handle if table == "own" else None, n, keys, select, ids, new_pos,
                                              C.byref(out) if n_ids == "out" else None)
    return st, (sess.lib.urcco_last_error() or b"").decode(), out.value


def refused_calls(sess, d, reserved_batch):
    """(name, the call's arguments, what the message must name) for every refusal a table of min_count 1 knows."""
    dummy, dummy32 = sess.empty(4, torch.int64), sess.empty(4, torch.int32)
    p, p32 = dummy.data_ptr(), dummy32.data_ptr()
    dk = D.dev_u64(sess, reserved_batch)
    n = len(reserved_batch)
    ids, new_pos = sess.empty(n, torch.int32), sess.empty(n, torch.int64)
    sel = [0] * n
    sel[0] = -1                                                          # another position masked: the reserved key still takes part
    ds = D.dev_i32(sess, sel)
    keep = (dk, ids, new_pos, ds, dummy, dummy32)                        # the tensors outlive the calls
    return keep, [("the reserved key", dict(n=n, keys=dk.data_ptr(), select=None, ids=ids.data_ptr(), new_pos=new_pos.data_ptr()), "reserved key"),
                  ("the reserved key, another position masked", dict(n=n, keys=dk.data_ptr(), select=ds.data_ptr(), ids=None, new_pos=new_pos.data_ptr()), "reserved key"),
                  ("n_ids + n beyond 2^31 - 1", dict(n=INT32_MAX - d.n_ids + 1, keys=p, select=None, ids=p32, new_pos=p), "2^31 - 1"),
                  ("n = 2^32 - 1", dict(n=(1 << 32) - 1, keys=p, select=None, ids=p32, new_pos=p), "2^32 - 2"),
                  ("n < 0", dict(n=-1, keys=p, select=None, ids=p32, new_pos=p), "bad argument"),
                  ("keys NULL", dict(n=2, keys=None, select=None, ids=p32, new_pos=p), "bad argument"),
                  ("new_pos NULL", dict(n=2, keys=p, select=None, ids=p32, new_pos=None), "bad argument"),
                  ("n_ids NULL", dict(n=2, keys=p, select=None, ids=p32, new_pos=p, n_ids=None), "bad argument"),
                  ("session NULL", dict(n=2, keys=p, select=None, ids=p32, new_pos=p, session=None), "bad argument"),
                  ("table NULL", dict(n=2, keys=p, select=None, ids=p32, new_pos=p, table=None), "bad argument")]


def case_refusals(sess, grows, repeat=1):
    """After each refusal: the lookups of all known keys, n_ids and the ids of a following valid extend are those of a run without the refused call.
    grows: the refused batch with the reserved key is long enough to need a rehash -- the table must come out of it as it went in."""
    start = ordinary(0, 400)
    fresh = ordinary(1000, 150 if grows else 40)
    mid = len(fresh) // 2
    reserved_batch = fresh[:mid] + [D.RESERVED] + start[:5] + fresh[mid:] + [D.RESERVED]      # new keys BEFORE and after the reserved one: none may stay
    assert (D.capacity(400 + len(reserved_batch)) > 1024) == grows
    follow = [fresh[3], start[9], fresh[1], ordinary(3000, 1)[0], fresh[3]]
    known = D.dev_u64(sess, start + fresh)
    want_known = np.asarray(list(range(400)) + [-1] * len(fresh), np.int32)
    want_follow, _ = walk_batches(start, [follow], [None])
    for _ in range(repeat):
        d = ingest.dictionary_build(sess, D.dev_u64(sess, start))
        try:
            keep, calls = refused_calls(sess, d, reserved_batch)
            for name, args, names in calls:
                st, msg, out = extend_status(sess, d, **args)
                assert st == _lib.BAD_ARG and names in msg, (name, st, msg)
                if "reserved" in names:
                    assert "2 selected" in msg, msg
                assert out == -7, (name, "*n_ids is not written")
                assert D.same(ingest.dictionary_lookup(sess, d, known), want_known), name
                d2 = ingest.dictionary_build(sess, D.dev_u64(sess, start))      # the same refusal, then a valid extend: as without the refused call
                try:
                    assert extend_status(sess, d2, **args)[0] == _lib.BAD_ARG
                    got_ids, got_new = d2.extend(D.dev_u64(sess, follow))
                    assert d2.n_ids == want_follow[0][2] == 403, name
                    assert D.same(got_ids, np.asarray(want_follow[0][0], np.int32)) and D.same(got_new, np.asarray(want_follow[0][1], np.int64)), name
                finally:
                    d2.close()
            assert d.n_ids == 400
            del keep
        finally:
            d.close()


def case_min_count_table_is_refused(sess):
    keys = [k for i, k in enumerate(ordinary(0, 30)) for _ in range(1 + i % 3)]
    ref = D.Ref(keys, None, 2)
    dk = D.dev_u64(sess, keys)
    d = ingest.dictionary_build(sess, dk, None, 2)
    try:
        ids, new_pos = sess.empty(len(keys), torch.int32), sess.empty(len(keys), torch.int64)
        for n in (len(keys), 0):                                         # an empty batch is refused all the same
            st, msg, out = extend_status(sess, d, n, dk.data_ptr(), None, ids.data_ptr(), new_pos.data_ptr())
            assert st == _lib.BAD_ARG and "min_count 2" in msg and out == -7, (st, msg)
        with pytest.raises(_lib.UrccoError):
            d.extend(dk)
        assert d.n_ids == ref.n_ids
        assert D.same(ingest.dictionary_lookup(sess, d, dk), np.asarray(ref.lookup(keys), np.int32))
    finally:
        d.close()


# ---- 9. the collision check ------------------------------------------------------------------------------------------------------------------------------------
def case_collisions(sess, repeat=1):
    rng = np.random.default_rng(11)
    pool = ordinary(0, 40)
    check_of = lambda keys: [D.mix(k ^ 0x5EED) for k in keys]
    start = [pool[int(i)] for i in rng.integers(0, 20, 300)]                 # the ids of the build: the first 20 keys of the pool
    batch = [pool[int(i)] for i in rng.integers(0, 40, 700)]
    old_victim = next(k for k in batch if k in start)
    new_victim = next(k for k in batch if k not in start)
    for victim in (old_victim, new_victim):
        for _ in range(repeat):
            check = check_of(batch)
            occ = [p for p, k in enumerate(batch) if k == victim]
            assert len(occ) >= 4
            planted = occ[1::2]                                              # a second string behind the same key: some of its LATER occurrences
            for p in planted:
                check[p] ^= 0x10
            d = ingest.dictionary_build(sess, D.dev_u64(sess, start)).with_check_keys(D.dev_u64(sess, check_of(start)))
            try:
                with pytest.raises(ingest.HashCollision) as ei:
                    d.extend(D.dev_u64(sess, batch), None, D.dev_u64(sess, check))
                assert ei.value.n_mismatch == len(planted)
                # the state a collision leaves: the batch is in the dictionary, check keys included; the clean stream passes afterwards
                want, ids = walk_batches(start, [batch], [None])
                assert d.n_ids == want[0][2]
                got_ids, got_new = d.extend(D.dev_u64(sess, batch), None, D.dev_u64(sess, check_of(batch)))
                assert D.same(got_ids, np.asarray(want[0][0], np.int32)) and int(got_new.numel()) == 0
                sel = [0] * len(batch)
                for p in planted:
                    sel[p] = -1                                              # the planted positions masked: nothing to report
                d.extend(D.dev_u64(sess, batch), D.dev_i32(sess, sel), D.dev_u64(sess, check))
                assert D.same(d.check_keys[: d.n_ids], np.asarray(check_of(sorted(ids, key=ids.get)), np.uint64).view(np.int64))
                with pytest.raises(ValueError):
                    d.extend(D.dev_u64(sess, batch))                         # check keys for every id or for none
            finally:
                d.close()
    d = ingest.dictionary_build(sess, D.dev_u64(sess, []))                  # from the empty table, growing the buffer of check keys batch by batch
    try:
        for lo in range(0, 40, 7):
            keys = pool[: lo + 7][::-1]
            d.extend(D.dev_u64(sess, keys), None, D.dev_u64(sess, check_of(keys)))
        assert d.n_ids == 40
    finally:
        d.close()


# ---- 10. arguments that are fine ---------------------------------------------------------------------------------------------------------------------------------
def case_nullable_ids_and_empty_batches(sess):
    start = ordinary(0, 10)
    d = ingest.dictionary_build(sess, D.dev_u64(sess, start))
    try:
        batch = D.dev_u64(sess, start[:3] + ordinary(50, 4))
        new_pos = sess.empty(7, torch.int64)
        st, msg, n_ids = extend_status(sess, d, 7, batch.data_ptr(), None, None, new_pos.data_ptr())      # ids NULL
        assert st == _lib.OK and n_ids == 14, (st, msg)
        assert D.host(new_pos[:4]) == [3, 4, 5, 6]
        assert D.host(ingest.dictionary_lookup(sess, d, batch)) == [0, 1, 2, 10, 11, 12, 13]
        st, msg, n_ids = extend_status(sess, d, 0, None, None, None, None)                                # n = 0: every pointer may be NULL
        assert st == _lib.OK and n_ids == 14, (st, msg)
    finally:
        d.close()
