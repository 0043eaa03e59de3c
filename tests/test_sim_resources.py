"""Nothing is left behind: every device allocation, pinned host allocation, event and stream the library creates is given back when the object
that owns it is destroyed.  The host simulator counts its live objects (tests/hostsim/hipsim.cpp, hipsim_live); a child process records the
counters, builds and tears down a session, a key table and contexts of every kind -- with the smallest shapes that reach every owned member:
three event types, a few hundred users, a few dozen items -- and finds the counters where they were after urcco_shutdown (which also trims the
pinned pool, so host allocations are held to the same standard).  Every case runs twice, and each checks just before its teardown that the objects
it is about were alive: a case that created nothing would prove nothing."""
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("device allocations", "host allocations", "events", "streams")
N_USERS = 300


def _mats():
    from helpers import rand_csr
    rng = np.random.default_rng(53)
    return [rand_csr(rng, N_USERS, 60, 5), rand_csr(rng, N_USERS, 30, 4), rand_csr(rng, N_USERS, 12, 2)]


def _host_datasets(mats):
    from universal_recommender_amd import _lib
    arr = (_lib.Dataset * len(mats))()
    for d, m in enumerate(mats):
        arr[d].matrix.n_rows, arr[d].matrix.n_cols = m.n_rows, m.n_cols
        arr[d].matrix.row_ptr, arr[d].matrix.col_idx = m.row_ptr.ctypes.data, m.col_idx.ctypes.data
        arr[d].max_elements_per_row, arr[d].max_interesting_elements = 500, 50
    return arr


def session_case(lib, held):
    """One plain session: the model build stage by stage (cco_rows in the LDS classes, then with a k only the dense global class serves), the recommend
    call without and with rules, the three history calls."""
    import torch
    import history_ref as H
    import recommend_ref as R
    import recommend_rules_ref as RR
    from helpers import to_dev, to_params
    from oracle import c_oracle as O
    from universal_recommender_amd.device import DeviceSession, cross_occurrence_device
    sess = DeviceSession(torch.device("cpu"), lib)
    sess.set_timing(True)                                     # the pooled timing events
    mats = _mats()
    for k in (50, 300):                                       # 300 > the multi-pass class's largest k: the session's dense counters
        out = cross_occurrence_device(sess, [to_dev(m, "cpu") for m in mats], to_params([O.DatasetParams(500, k, None)] * 3), 3)
        sess.synchronize()
        assert all(int(o.stats[0]) > 0 for o in out)
    assert sess.expand_form() >= 0
    p = R.make_problem(11, 40, 30, cols=(40, 60, 7), boosts=(1.05, 20.0, 0.3), k=10, hist_hi=12, hub_cols=(0,))
    dr = RR.DeviceRules(R.DeviceProblem(sess, p), RR.make_rules(p, 3))
    for names in (None, ("any", "none", "range", "ind")):
        count, *_ = dr.run(names, 10)
        assert count.max() > 0
    hp = H.make_problem(n_users=N_USERS, cols=(40, 60, 7), heavy=100, planted=(0, 1, 63, 64, 65))
    hd = H.DeviceProblem(sess, hp)                            # urcco_dev_history_index per stream
    terms, excl, _ = sess.history_rows(hd.q_users, hp.n_users, hd.events([5] * 3), hp.n_items, hd.extra)   # _bounds, then _rows
    sess.synchronize()
    assert int(excl[0][-1]) > 0 and all(int(rp[-1]) > 0 for rp, _ in terms)
    dev, _, events, streams = held()
    assert dev >= 7 and events >= 2 and streams == 1, (dev, events, streams)   # arena, two xLogX tables, form word, three dense-class arrays; timing events
    sess.close()


def key_table_case(lib, held):
    import torch
    from universal_recommender_amd import ingest
    from universal_recommender_amd.device import DeviceSession
    sess = DeviceSession(torch.device("cpu"), lib)
    keys = torch.from_numpy(np.random.default_rng(1).integers(0, 50, 400).astype(np.int64))
    d = ingest.dictionary_build(sess, keys)
    assert 0 < d.n_ids <= 50
    assert int(ingest.dictionary_lookup(sess, d, keys).min()) >= 0
    before = held()[0]
    d.close()
    assert held()[0] == before - 4                            # keys, first positions, counts, ids
    sess.close()


def one_gpu_context_case(lib, held):
    """urcco_context_stage / _finish on a one-GPU context: staging rings, the builder thread, the pinned result blocks."""
    from universal_recommender_amd import _lib
    from universal_recommender_amd.device import Context
    mats = _mats()
    arr, n = _host_datasets(mats), len(mats)
    ctx = Context("cpu", lib)
    for _ in range(2):
        out = (_lib.Indicators * n)()
        _lib.check(lib.urcco_context_stage(ctx.handle, arr, n, 3), lib)
        _lib.check(lib.urcco_context_finish(ctx.handle, out, None), lib)
        assert all(int(out[d].nnz) > 0 for d in range(n))
        lib.urcco_free_indicators(out, n)
    dev, host, events, streams = held()
    # an arena and the staged / sampled / output buffers per event type; host: the staging ring and a mapped word per event type; five events per
    # event type, four of the device and the ring's slots; a stream per event type
    assert dev >= 9 * n and host >= 1 + n and events > 5 * n + 4 and streams == n, (dev, host, events, streams)
    ctx.close()


def emulated_ranks_case(lib, held):
    """Four ranks on one device through the exchange path: the exchange buffers of every event type, the primary's CSC fragments, the row filter."""
    import torch
    from helpers import shard_rows, to_dev, to_params
    from oracle import c_oracle as O
    from universal_recommender_amd import _lib, sharded
    from universal_recommender_amd.device import Context
    W = 4
    mats = _mats()
    n = len(mats)
    shards, cuts = shard_rows([to_dev(m, "cpu") for m in mats], W)
    coll = sharded.DeviceLoopbackCollectives(W, "cpu")
    ctx = Context(torch.device("cpu"), lib, n_gpus=W, flags=_lib.FLAG_EMULATE_RANKS, collectives=coll)
    for _ in range(2):
        ctx.build(shards, to_params([O.DatasetParams(30, 10, None)] * 3), 3, N_USERS, cuts[:-1])
        res = ctx.results()
        assert coll.error is None
        assert sum(int(ind.stats[0]) for row in res for ind in row) > 0
    res = None
    dev, _, events, streams = held()
    # per rank and event type: an arena and at least the eight exchange buffers (row lengths, sizes, masks, offsets, totals, packed rows, the received
    # CSR); five events per event type and four per rank; ONE stream, the emulation stream every session of every rank borrows
    assert dev >= 9 * W * n and events == W * (5 * n + 4) and streams == 1, (dev, events, streams)
    ctx.close()


def abandoned_stage_case(lib, held):
    """A context destroyed with a staged build nobody finished."""
    from universal_recommender_amd import _lib
    from universal_recommender_amd.device import Context
    mats = _mats()
    arr, n = _host_datasets(mats), len(mats)
    ctx = Context("cpu", lib)
    _lib.check(lib.urcco_context_stage(ctx.handle, arr, n, 3), lib)
    assert held()[0] > 0
    ctx.close()


CASES = (session_case, key_table_case, one_gpu_context_case, emulated_ranks_case, abandoned_stage_case)


def child():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from hostsim import build_sim
    from universal_recommender_amd import _lib
    lib = _lib.load(build_sim.build())
    lib.hipsim_live.restype = C.c_longlong
    lib.hipsim_live.argtypes = [C.c_int]

    def live():
        gc.collect()
        assert lib.urcco_shutdown() == 0        # the default context (none here) and the unused blocks of the pinned pool
        return [int(lib.hipsim_live(k)) for k in range(len(KINDS))]

    base = live()
    print("live at the start:", dict(zip(KINDS, base)), flush=True)
    failures = []
    for case in CASES:
        for rep in (1, 2):
            case(lib, lambda: [int(lib.hipsim_live(k)) for k in range(len(KINDS))])
            now = live()
            print(f"{case.__name__} run {rep}:", dict(zip(KINDS, now)), flush=True)
            failures += [f"{case.__name__} run {rep}: {now[k] - base[k]:+d} {KINDS[k]}" for k in range(len(KINDS)) if now[k] != base[k]]
    assert not failures, failures
    print("nothing left behind", flush=True)


def test_nothing_is_left_behind(sim_lib):
    env = {k: v for k, v in os.environ.items() if k not in ("HIPSIM_GUARD", "HIPSIM_DEVICE_COUNT")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "nothing left behind" in r.stdout, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"


if __name__ == "__main__":
    child()
