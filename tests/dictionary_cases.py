"""The device dictionary (csrc/ingest_kernels.hip: ig_insert / ig_first_flags / ig_assign / ig_lookup / ig_verify) on CONSTRUCTED keys, shared by
test_sim_dictionary.py and test_gpu_dictionary.py.  The four entry points are called directly (ingest.dictionary_build / _lookup / _verify /
_verify_against), never through prepare_device, and every result is compared exactly with a Python dict walked in stream order.

Keys are not hashed: the table's hash (ig_mix, the splitmix64 finaliser) and its capacity rule are written out again here, and `keys_at` inverts the
finaliser, so a case decides which slot each of its keys calls home -- probe chains of hundreds of slots, a chain that wraps from the last slot to slot 0,
64 different keys of one wave on one empty slot.  test_sim_dictionary.py (without a device) reads the constants out of the sources and compares
them with the ones below: a change of the hash cannot quietly turn these cases back into random ones.

One test of the kernels has no observable effect and no case here can fail without it: `select` in ig_first_flags_kernel.  The insert pass has
already left masked positions out, so the position minimum of a masked position's slot is another position, or still ~0 for a slot nobody claimed --
and no position equals that, which is what the bound of 2^32 - 2 events is for.

`repeat` (the hardware driver): the whole case runs that many times; every run must give the same tables of ids."""
import ctypes as C

import numpy as np
import torch

from universal_recommender_amd import _lib, ingest

# ---- the table's hash and capacity, restated ---------------------------------------------------------------------------------------------------------
MIX_SHIFTS = (30, 27, 31)
MIX_MULTIPLIERS = (0xBF58476D1CE4E5B9, 0x94D049BB133111EB)
MIN_CAPACITY = 1024
SCAN_TILE = 2048
RESERVED = (1 << 64) - 1          # IG_EMPTY: the "empty slot" value
M64 = (1 << 64) - 1


def mix(x: int) -> int:
    for i, sh in enumerate(MIX_SHIFTS):
        x ^= x >> sh
        if i < 2:
            x = (x * MIX_MULTIPLIERS[i]) & M64
    return x


def unmix(h: int) -> int:
    def unshift(x, sh):           # inverse of x ^= x >> sh
        y = x
        for _ in range(64 // sh):
            y = x ^ (y >> sh)
        return y
    h = unshift(h, MIX_SHIFTS[2])
    h = (h * pow(MIX_MULTIPLIERS[1], -1, 1 << 64)) & M64
    h = unshift(h, MIX_SHIFTS[1])
    h = (h * pow(MIX_MULTIPLIERS[0], -1, 1 << 64)) & M64
    return unshift(h, MIX_SHIFTS[0])


def capacity(n: int) -> int:
    cap = MIN_CAPACITY
    while cap < 2 * n:
        cap <<= 1
    return cap


def home(key: int, cap: int) -> int:
    return mix(key) & (cap - 1)


def keys_at(slot: int, cap: int, count: int, skip: int = 0):
    """`count` distinct keys whose home slot in a table of `cap` slots is `slot` (the keys number skip, skip + 1, ... of that slot; never the reserved one)."""
    bits = cap.bit_length() - 1
    out, j = [], skip
    while len(out) < count:
        upper = ((j + 1) * 0x9E3779B97F4A7C15) & (M64 >> bits)      # distinct for distinct j (an odd multiplier), spread over all the upper bits
        k = unmix(upper << bits | slot)
        j += 1
        if k != RESERVED:
            out.append(k)
    assert all(home(k, cap) == slot for k in out) and len(set(out)) == count
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
def walk(keys, select):
    """(first selected position, selected occurrences) per key."""
    first, count = {}, {}
    for p, k in enumerate(keys):
        if select is not None and select[p] < 0:
            continue
        if k not in first:
            first[k] = p
            count[k] = 0
        count[k] += 1
    return first, count


class Ref:
    """A dict walked in stream order over the positions whose select is not negative."""

    def __init__(self, keys, select, min_count, walked=None):
        need = max(int(min_count), 1)
        first, count = walked or walk(keys, select)
        kept = sorted((p, k) for k, p in first.items() if count[k] >= need)     # by first position
        self.ids = {k: i for i, (_, k) in enumerate(kept)}
        self.first_pos = [p for p, _ in kept]
        self.n_ids = len(kept)

    def lookup(self, keys, select=None):
        return [-1 if (select is not None and select[p] < 0) else self.ids.get(k, -1) for p, k in enumerate(keys)]

    def verify(self, keys, select, check, dict_check):
        bad = 0
        for p, k in enumerate(keys):
            if select is not None and select[p] < 0:
                continue
            i = self.ids.get(k)
            if i is not None and check[p] != dict_check[self.first_pos[i]]:
                bad += 1
        return bad


# ---- device side ---------------------------------------------------------------------------------------------------------------------------------------
def dev_u64(sess, keys):
    """Python ints in [0, 2^64) -> the int64 bit patterns, in a tensor of the session (under guard pages: one that ends at a guard page)."""
    a = np.asarray(keys, dtype=np.uint64).view(np.int64)
    t = sess.empty(a.size, torch.int64)
    t.copy_(torch.from_numpy(a))
    return t


def dev_i32(sess, v):
    if v is None:
        return None
    a = np.asarray(v, dtype=np.int32)
    t = sess.empty(a.size, torch.int32)
    t.copy_(torch.from_numpy(a))
    return t


def host(t):
    return t.cpu().numpy().tolist()


def same(t, want):
    return np.array_equal(t.cpu().numpy(), want)


def check_stream(sess, keys, select=None, min_count=1, queries=(), repeat=1, ref=None):
    """Build from (keys, select, min_count); n_ids, first_pos, the ids of the stream's own positions (with and without select) and of `queries` == Ref.
    Returns (Ref, ids of the stream) of the last run."""
    keys = [int(k) for k in keys]
    ref = ref or Ref(keys, select, min_count)
    dk, ds, dq = dev_u64(sess, keys), dev_i32(sess, select), dev_u64(sess, queries)
    want_sel, want_all, want_q = (np.asarray(x, np.int32) for x in (ref.lookup(keys, select), ref.lookup(keys), ref.lookup(list(queries))))
    want_first = np.asarray(ref.first_pos, np.int64)
    for run in range(repeat):              # every run equals the one restatement, hence every other run
        d = ingest.dictionary_build(sess, dk, ds, min_count)
        try:
            assert d.n_ids == ref.n_ids, (run, d.n_ids, ref.n_ids)
            assert same(d.first_pos, want_first), run
            assert same(ingest.dictionary_lookup(sess, d, dk, ds), want_sel), run
            assert same(ingest.dictionary_lookup(sess, d, dk), want_all), run
            assert same(ingest.dictionary_lookup(sess, d, dq), want_q), run
        finally:
            d.close()
    return ref, want_sel.tolist()


def mask_third(rng, keys, force_first_of=8):
    """select: about a third of the positions negative -- among them the FIRST appearance of `force_first_of` keys; the others >= 0 (0 included)."""
    n = len(keys)
    sel = rng.integers(0, 1000, n).astype(np.int32)
    sel[:: 7] = 0
    sel[rng.random(n) < 1 / 3] = -1
    firsts = {}
    for p, k in enumerate(keys):
        firsts.setdefault(k, p)
    pos = sorted(firsts.values())
    for p in pos[:: max(len(pos) // max(force_first_of, 1), 1)][:force_first_of]:
        sel[p] = -1 - (p % 3)
    return sel.tolist()


def both(sess, keys, min_count=1, queries=(), repeat=1, seed=0):
    """The stream unmasked and once with about a third of it masked."""
    check_stream(sess, keys, None, min_count, queries, repeat)
    if len(keys):
        check_stream(sess, keys, mask_third(np.random.default_rng(seed + 1000), keys), min_count, queries, repeat)


# ---- 1. a long chain that wraps -------------------------------------------------------------------------------------------------------------------------
def chain_stream(home_slot, seed=1, distinct=300):
    """300 distinct keys of ONE home slot in a table of 1024 slots: 150 once, 100 twice, 50 three times (500 positions: the table stays at 1024), shuffled."""
    rng = np.random.default_rng(seed)
    cap = MIN_CAPACITY
    ks = keys_at(home_slot, cap, distinct)
    reps = [1] * (distinct // 2) + [2] * (distinct // 3) + [3] * (distinct - distinct // 2 - distinct // 3)
    stream = [k for k, r in zip(ks, reps) for _ in range(r)]
    stream = [stream[i] for i in rng.permutation(len(stream))]
    assert capacity(len(stream)) == cap
    return ks, stream


def case_chain_that_wraps(sess, repeat=1):
    cap = MIN_CAPACITY
    ks, stream = chain_stream(cap - 1)                     # slots 1023, 0, 1, ..., 298
    absent = keys_at(cap - 1, cap, 50, skip=len(ks) + 10)    # walk the whole chain, over the wrap, to the first free slot
    absent += [k for s in (0, 1, 100, 297, 298, 299) for k in keys_at(s, cap, 2)]   # start inside the chain / on its last slot / just behind it
    assert not set(absent) & set(ks)
    both(sess, stream, 1, ks + absent, repeat, seed=1)
    both(sess, stream, 2, ks + absent, repeat, seed=2)


# ---- 2. one wave, one slot -----------------------------------------------------------------------------------------------------------------------------
def wave_stream(base):
    """Positions base .. base + 63: 64 distinct keys of one home slot; base + 64 .. base + 127: the same keys in reverse order; before base: 16 ordinary keys."""
    n = base + 128
    cap = capacity(n)
    ks = keys_at(5, cap, 64)
    fill = [(0x1000 + (i % 16)) for i in range(base)]
    return fill + ks + ks[::-1]


def case_one_wave_one_slot(sess, base, repeat=1):
    stream = wave_stream(base)
    ref, _ = check_stream(sess, stream, None, 1, (), repeat)
    assert ref.first_pos[-64:] == list(range(base, base + 64))     # ids in position order, whoever won the slot
    check_stream(sess, stream, None, 2, (), repeat)
    check_stream(sess, stream, mask_third(np.random.default_rng(base + 3), stream, 40), 1, (), repeat)
    # every first appearance of the forward block masked: the reversed block holds the firsts, in the opposite key order
    sel = [0] * len(stream)
    for p in range(base, base + 64):
        sel[p] = -1
    ref, _ = check_stream(sess, stream, sel, 1, (), repeat)
    assert ref.first_pos[-64:] == list(range(base + 64, base + 128))


# ---- 3. a hot key, counts exactly below, at and above min_count --------------------------------------------------------------------------------------------
def hot_stream(hot, threshold, per_count, masked, seed=7):
    """One key `hot` times, per_count ordinary keys each with exactly 1, 2, threshold - 1, threshold, threshold + 1 SELECTED occurrences, shuffled.
    masked: every key gets half as many occurrences again at masked positions (they must not count); else select is None."""
    rng = np.random.default_rng(seed)
    counts = [1, 2, threshold - 1, threshold, threshold + 1]
    key_ids = np.arange(1 + per_count * len(counts), dtype=np.int64)
    reps = np.concatenate([[hot], np.repeat(counts, per_count)])
    who = np.repeat(key_ids, reps)
    sel = np.zeros(who.size, np.int32)
    if masked:
        extra = np.repeat(key_ids, (reps + 1) // 2)
        who = np.concatenate([who, extra])
        sel = np.concatenate([sel + 1, np.full(extra.size, -1, np.int32)])
    order = rng.permutation(who.size)
    who, sel = who[order], sel[order]
    table = np.array([unmix(0x51ED270B0000 + 977 * i) for i in range(key_ids.size)], dtype=np.uint64)    # arbitrary distinct keys
    assert RESERVED not in table and np.unique(table).size == table.size
    return table[who].tolist(), (sel.tolist() if masked else None), dict(zip(table.tolist(), reps.tolist()))


def case_hot_key(sess, hot=200_000, threshold=1000, per_count=200, repeat=1):
    for masked in (False, True):
        keys, sel, selected = hot_stream(hot, threshold, per_count, masked)
        walked = walk(keys, sel)
        for min_count in (1, 2, threshold):
            ref = Ref(keys, sel, min_count, walked)
            assert ref.n_ids == sum(1 for c in selected.values() if c >= min_count)     # the threshold sits where the construction put it
            check_stream(sess, keys, sel, min_count, (), repeat, ref=ref)


# ---- 4. sizes ------------------------------------------------------------------------------------------------------------------------------------------
def case_sizes(sess, repeat=1):
    queries = [unmix(i + 1) for i in range(100)]
    ref, _ = check_stream(sess, [], None, 1, queries, repeat)
    assert ref.n_ids == 0
    both(sess, [12345], 1, queries, repeat)
    check_stream(sess, [12345], None, 2, queries, repeat)              # the only key below min_count
    for n in (512, 513):                                               # the capacity doubles between them
        keys = [unmix(1000 + i) for i in range(n)]
        assert capacity(n) == (1024 if n == 512 else 2048)
        both(sess, keys, 1, queries, repeat, seed=n)
    keys = [unmix(i % 37) for i in range(300)]
    ref, ids = check_stream(sess, keys, [-1] * 300, 1, queries, repeat)   # every position masked
    assert ref.n_ids == 0 and set(ids) == {-1}
    for min_count in (0, -3):                                          # both mean 1
        ref, _ = check_stream(sess, keys + [99991], None, min_count, queries, repeat)
        assert ref.n_ids == 38


# ---- 5. first positions on the edges of the scan's tiles -------------------------------------------------------------------------------------------------
def case_tile_edges(sess, repeat=1):
    n = 3 * SCAN_TILE + 5
    firsts = [0, SCAN_TILE - 1, SCAN_TILE, 2 * SCAN_TILE - 1, 2 * SCAN_TILE, n - 1]
    rng = np.random.default_rng(5)
    keys, seen = [], []
    for p in range(n):
        if p in firsts:
            seen.append(unmix(77 + len(seen)))
            keys.append(seen[-1])
        else:
            keys.append(seen[int(rng.integers(len(seen)))])
    ref, _ = check_stream(sess, keys, None, 1, (), repeat)
    assert ref.first_pos == firsts
    check_stream(sess, keys, None, 2, (), repeat)                      # the key of the last position occurs once
    check_stream(sess, keys, mask_third(np.random.default_rng(6), keys, 3), 1, (), repeat)


# ---- 6. extreme keys -------------------------------------------------------------------------------------------------------------------------------------
EXTREME = [0, 1, 1 << 63, (1 << 64) - 2]


def case_extreme_keys(sess, repeat=1):
    rng = np.random.default_rng(8)
    keys = [EXTREME[int(i)] for i in rng.integers(0, 4, 200)]
    both(sess, keys, 1, EXTREME + [2, (1 << 63) - 1, (1 << 63) + 1, (1 << 64) - 3], repeat)
    ref, _ = check_stream(sess, EXTREME, None, 1, EXTREME, repeat)
    assert ref.n_ids == 4


# ---- 7. the reserved key ---------------------------------------------------------------------------------------------------------------------------------
def reserved_streams():
    """(name, stream, positions of the reserved key)."""
    cap = MIN_CAPACITY
    h = home(RESERVED, cap)
    ks, chain = chain_stream((h - 150) & (cap - 1), seed=9)       # the reserved key's home slot lies in the middle of this chain
    mid = len(chain) // 2
    return [("alone", [RESERVED], [0]),
            ("before a key of its home slot", [RESERVED, keys_at(h, cap, 1)[0]], [0]),
            ("twice before keys of its home slot", [RESERVED, RESERVED] + keys_at(h, cap, 3), [0, 1]),
            ("in the middle of a chain", chain[:mid] + [RESERVED] + chain[mid:], [mid])]


def build_status(sess, keys, select, min_count=1):
    """urcco_dev_dictionary_build called directly: (status, message, table handle, n_ids)."""
    dk, ds = dev_u64(sess, keys), dev_i32(sess, select)
    first_pos = sess.empty(max(len(keys), 1), torch.int64)
    handle, n_ids = C.c_void_p(0xDEAD0), C.c_int64(-7)
    st = sess.lib.urcco_dev_dictionary_build(sess.handle, len(keys), dk.data_ptr(), None if ds is None else ds.data_ptr(), min_count, first_pos.data_ptr(),
                                             C.byref(handle), C.byref(n_ids))
    msg = (sess.lib.urcco_last_error() or b"").decode()
    return st, msg, handle, n_ids.value


def case_reserved_key(sess, name, repeat=1):
    stream, where = next((s, w) for n, s, w in reserved_streams() if n == name)
    for _ in range(repeat):
        st, msg, handle, _ = build_status(sess, stream, None)
        if st == _lib.OK:
            sess.lib.urcco_key_table_destroy(handle)
        assert st == _lib.BAD_ARG and "reserved key" in msg and f"{len(where)} selected" in msg, (st, msg)
        assert handle.value is None, "no table is handed out"
        sel = [3] * len(stream)                                      # another position masked: still refused
        sel[-1] = -1
        if len(stream) - 1 not in where:
            assert build_status(sess, stream, sel)[0] == _lib.BAD_ARG
    # with its positions masked the reserved key is ignored: the stream equals the restatement, the lookup answers -1 for the key (selected or not),
    # and verify skips it whatever its check key
    sel = [0] * len(stream)
    for p in where:
        sel[p] = -1
    ref, _ = check_stream(sess, stream, sel, 1, [RESERVED, RESERVED - 1], repeat)
    assert RESERVED not in ref.ids
    dk, ds = dev_u64(sess, stream), dev_i32(sess, sel)
    check = [mix(k ^ 0xABCDEF) for k in stream]
    for p in where:
        check[p] = 1
    dc = dev_u64(sess, check)
    d = ingest.dictionary_build(sess, dk, ds, 1)
    try:
        assert ingest.dictionary_verify(sess, d, dk, dc, ds) == 0
        assert ingest.dictionary_verify(sess, d, dk, dc, None) == 0
        assert ingest.dictionary_verify_against(sess, d, dk, dc, dc) == 0
    finally:
        d.close()


# ---- 8. verify / verify_against ----------------------------------------------------------------------------------------------------------------------------
def case_verify(sess, repeat=1):
    rng = np.random.default_rng(11)
    pool = [unmix(500 + i) for i in range(40)]
    keys = [pool[int(i)] for i in rng.integers(0, 40, 700)]
    check = [mix(k ^ 0x5EED) for k in keys]
    victim = keys[3]
    occ = [p for p, k in enumerate(keys) if k == victim]
    assert len(occ) >= 6
    planted = occ[2::2]                                               # a second string behind the same key: some of its later occurrences
    for p in planted:
        check[p] ^= 0x10
    # a second stream looked up in the first one's dictionary: unknown keys (skipped) and one known key with a foreign check key
    keys2 = [pool[int(i)] for i in rng.integers(0, 40, 300)] + [unmix(900 + i) for i in range(30)]
    keys2 = [keys2[i] for i in rng.permutation(len(keys2))]
    check2 = [mix(k ^ 0x5EED) for k in keys2]
    victim2 = next(k for k in keys2 if k in pool and k != victim)
    planted2 = [p for p, k in enumerate(keys2) if k == victim2]
    for p in planted2:
        check2[p] ^= 0x20
    dk, dc, dk2, dc2 = dev_u64(sess, keys), dev_u64(sess, check), dev_u64(sess, keys2), dev_u64(sess, check2)
    sel_all = mask_third(np.random.default_rng(12), keys, 5)
    sel_planted = [0] * len(keys)
    for p in planted[:-1]:
        sel_planted[p] = -1                                           # all but one colliding position masked
    sel_first = [0] * len(keys)
    sel_first[occ[0]] = sel_first[occ[1]] = -1                        # the victim's first selected occurrence is now a PLANTED one: the clean ones mismatch
    sel2 = [0] * len(keys2)
    for p in planted2[1:]:
        sel2[p] = -1
    for _ in range(repeat):
        for sel, want in ((None, len(planted)), (sel_planted, 1), (sel_all, None), (sel_first, len(occ) - 2 - len(planted))):
            ref = Ref(keys, sel, 1)
            n = ref.verify(keys, sel, check, check)
            assert want is None or n == want, (n, want)
            d = ingest.dictionary_build(sess, dk, dev_i32(sess, sel), 1)
            try:
                assert ingest.dictionary_verify(sess, d, dk, dc, dev_i32(sess, sel)) == n
                if sel is None or sel is sel_planted:                 # the other stream against this dictionary
                    base = ref.verify(keys2, None, check2, check)
                    assert base == len(planted2)
                    assert ingest.dictionary_verify_against(sess, d, dk2, dc2, dc) == base
                    assert ingest.dictionary_verify_against(sess, d, dk2, dc2, dc, dev_i32(sess, sel2)) == ref.verify(keys2, sel2, check2, check) == 1
            finally:
                d.close()
        # min_count: a key without an id is not verified
        ref = Ref(keys, None, len(occ) + 1)
        assert victim not in ref.ids
        d = ingest.dictionary_build(sess, dk, None, len(occ) + 1)
        try:
            assert ingest.dictionary_verify(sess, d, dk, dc) == ref.verify(keys, None, check, check) == 0
        finally:
            d.close()


# ---- 9. arguments ------------------------------------------------------------------------------------------------------------------------------------------
def case_arguments(sess):
    lib, dummy = sess.lib, sess.empty(4, torch.int64)
    p = dummy.data_ptr()
    handle, n_ids = C.c_void_p(), C.c_int64()
    calls = {"n = 2^32 - 1": (sess.handle, (1 << 32) - 1, p, None, 1, p, C.byref(handle), C.byref(n_ids)),
             "n < 0": (sess.handle, -1, p, None, 1, p, C.byref(handle), C.byref(n_ids)),
             "table NULL": (sess.handle, 2, p, None, 1, p, None, C.byref(n_ids)),
             "n_ids NULL": (sess.handle, 2, p, None, 1, p, C.byref(handle), None),
             "keys NULL": (sess.handle, 2, None, None, 1, p, C.byref(handle), C.byref(n_ids)),
             "session NULL": (None, 2, p, None, 1, p, C.byref(handle), C.byref(n_ids))}
    for what, args in calls.items():
        assert lib.urcco_dev_dictionary_build(*args) == _lib.BAD_ARG, what
        assert handle.value is None, what
        if what == "n = 2^32 - 1":
            assert "2^32 - 2" in (lib.urcco_last_error() or b"").decode()
    bad = C.c_int64()
    assert lib.urcco_dev_dictionary_lookup(sess.handle, None, 2, p, None, p) == _lib.BAD_ARG
    assert lib.urcco_dev_dictionary_verify(sess.handle, None, 2, p, None, p, p, C.byref(bad)) == _lib.BAD_ARG
    d = ingest.dictionary_build(sess, dev_u64(sess, [1, 2]), None, 1)
    try:
        assert lib.urcco_dev_dictionary_lookup(sess.handle, d.handle, -1, p, None, p) == _lib.BAD_ARG
        assert lib.urcco_dev_dictionary_verify(sess.handle, d.handle, 2, p, None, p, p, None) == _lib.BAD_ARG
        assert lib.urcco_dev_dictionary_verify_against(sess.handle, d.handle, 2, p, None, p, None, p, C.byref(bad)) == _lib.BAD_ARG
        assert host(ingest.dictionary_lookup(sess, d, dev_u64(sess, []))) == []        # n = 0 against a live table
    finally:
        d.close()


RESERVED_NAMES = [n for n, _, _ in reserved_streams()]
