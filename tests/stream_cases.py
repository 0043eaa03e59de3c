"""The stream contract of the session level (the DeviceSession docstring): every launch, copy, memset and event record of a urcco_dev_* call
names the session's stream, and every torch op of the Python layer runs on torch's current stream -- which the caller makes the session's stream.  Shared by
tests/test_sim_streams.py (the simulator's null-stream audit) and tests/test_gpu_streams.py (the library on a caller's non-blocking stream).

FAMILIES: per family of the session level one existing case of the case libraries, as it stands there, with its own reference and its own (exact) comparison.
PROTOCOL: the stale-data protocol's call sets -- a problem A on the device, a problem B of the same sizes staged next to it, and the numpy references of both.
B is A with the query (or event) order reversed, so every size argument is equal and every index of either problem is in range for the other."""
import functools
import time

import numpy as np
import torch

from universal_recommender_amd import _lib

# The delay the protocol enqueues in front of the copies of B, in milliseconds of device time: the ceiling the contract's test allows.  It has to outlast the
# host-side enqueue of the slowest call set twenty times over; profiles/stream_contract_first_run.log holds the enqueue times measured on the MI355X (the
# largest: well under a millisecond) and the cycle count this gave.  The guard is not this number but the `side.query() is False` of every case.
DELAY_MS = 50.0


# ---- one existing case per family ------------------------------------------------------------------------------------------------------------------
def _build(sess, mp):
    from test_sim_kernel_logic import test_small_three_events_all_modes
    test_small_three_events_all_modes(sess)                       # column counts, row scan, transpose, expand, rows, compaction: helpers.compare_with_oracle


def _llr(sess, mp):
    from test_gpu_parity import test_llr_and_rng_device_functions
    test_llr_and_rng_device_functions(sess)


def _hashed(sess, mp):
    import recommend_hashed_cases as H
    H.three(H.Context(sess, mp), 20)                              # LDS, hashed and dense under SMALL, all sixteen switch sets


def _forms(sess, mp):
    import recommend_hashed_cases as H
    H.three_form(H.Context(sess, mp), "rules")
    H.three_form(H.Context(sess, mp), "idf")                      # idf_weights, read back, and the weighted call


def _driven(sess, mp):
    import recommend_driven_cases as D
    D.mixed(D.H.Context(sess, mp), 20, True)                      # all four classes in one call


def _explain(sess, mp):
    import explain_ref as X
    X.check(sess, *X.edges(5))


def _audience(sess, mp):
    import audience_cases as A
    A.check_case(sess, (4, 65, 5, 7))
    A.check_case(sess, (8, 300, 65, 9))


def _quota(sess, mp):
    import quota_cases as Q
    Q.check_case(sess, Q.CASES[2], None)
    Q.check_case(sess, Q.CASES[11], 64)                           # 128 candidates a row against a table of 64 slots: the global tier


def _item_rows(sess, mp):
    import items_ref as I
    I.check(I.DeviceProblem(sess, I.make_problem()), [64])


def _history_rows(sess, mp):
    import history_ref as H
    H.check(H.DeviceProblem(sess, H.make_problem()), [5] * 3)     # history_index in the constructor, bounds + rows in the check


def _history_append(sess, mp):
    import history_append_cases as A
    A.edge_case(sess, A.make_edge_problem())


def _history_trim(sess, mp):
    import history_trim_cases as T
    T.chain_case(sess)                                            # trim, append, trim


def _history_cap(sess, mp):
    import history_cap_cases as C
    C.independence_case(sess)


def _history_dedup(sess, mp):
    import history_dedup_cases as D
    case = D.CASES[0]
    case[0](sess, "last", *case[1])


def _history_matrix(sess, mp):
    import history_matrix_cases as M
    M.window_cases(sess)                                          # history_users and history_matrix under a window


def _history_ranks(sess, mp):
    import history_ranks_cases as R
    R.id_cases(sess)


def _fill_order(sess, mp):
    import history_ranks_cases as R
    R.fill_digit_cases(sess)


def _props(sess, mp):
    import props_cases as PC
    PC.tie_cases(sess)                                            # apply, delete, rows, dates, exists through check_store


def _props_compact(sess, mp):
    import props_compact_cases as CC
    CC.twin_case(sess)


def _dictionary(sess, mp):
    import dictionary_cases as D
    D.case_one_wave_one_slot(sess, 0)


def _dictionary_extend(sess, mp):
    import dictionary_extend_cases as X
    X.case_batching(sess, 2)


def _metrics(sess, mp):
    import eval_ref as E
    E.check_problem(sess, 20)
    E.check_alignment(sess)                                       # tree_sum


def _preparator(sess, mp):
    from test_sim_ingest import test_prepare_handmade_and_degenerate_streams
    test_prepare_handmade_and_degenerate_streams(sess)


def _lifecycle(sess, mp):
    import history_lifecycle_cases as L
    L.run(sess, L.stack_for(sess), L.make_dense_schedule())


def _user_recommendations(sess, mp):
    from test_explain_predict import test_user_recommendations_rows_are_batch_predict_s
    from test_recommend_rules_golden import _stack
    from universal_recommender_amd.history import DeviceHistory
    algo, model, _, history, *_ = _stack(sess)
    test_user_recommendations_rows_are_batch_predict_s((algo, model, history, DeviceHistory.from_dict(sess, model, history)))   # explain=3, chunk=2


def _evaluate(sess, mp):
    import eval_ref as E
    E.check_evaluate(E.Stack(sess))                               # chunks of 64, 100 and 65536


FAMILIES = {"build stages": _build, "llr": _llr, "recommend lds+hashed+dense": _hashed, "recommend rules, weights, idf_weights": _forms, "recommend driven": _driven,
            "explain": _explain, "audience": _audience, "quota_cut": _quota, "item_rows": _item_rows, "history_index, history_rows": _history_rows,
            "history_append": _history_append, "history_trim": _history_trim, "history_cap": _history_cap, "history_dedup": _history_dedup,
            "history_users, history_matrix": _history_matrix, "history_ranks": _history_ranks, "fill_order": _fill_order,
            "props apply, delete, rows, dates, exists": _props, "props_compact": _props_compact, "dictionary build": _dictionary,
            "dictionary extend": _dictionary_extend, "rank_metrics, tree_sum": _metrics, "preparator": _preparator, "history lifecycle": _lifecycle,
            "user_recommendations": _user_recommendations, "evaluate": _evaluate}


# ---- the stale-data protocol ------------------------------------------------------------------------------------------------------------------------
def rev_csr(rp, ci):
    """the CSR with its rows in reverse order: the same lengths and entries, so the same nnz"""
    rows = np.split(ci[: rp[-1]], rp[1:-1])[::-1] if rp.size > 1 else []
    out = np.zeros_like(rp)
    np.cumsum(np.diff(rp)[::-1], out=out[1:])
    return out, np.concatenate(rows).astype(ci.dtype) if len(rows) and rp[-1] else ci[:0]


def host(out):
    return tuple(None if t is None else t.cpu().numpy() for t in out)


class CallSet:
    """inputs: (device tensor, numpy array of B) pairs -- the tensors hold A; call(sess) -> output tensors; want_a / want_b and compare(got, want): the
    references and the case library's exact comparison; syncs: the call synchronises by design, so only its first phase runs under the delay; before(sess):
    an earlier phase of the call set, run on A in front of the delay, whose result call(sess, result) takes -- want_b is then the reference of that mix."""

    def __init__(self, name, sess, inputs, call, want_a, want_b, compare, differ, syncs, before=None):
        self.name, self.call, self.want_a, self.want_b, self.compare, self.syncs, self.before = name, call, want_a, want_b, compare, syncs, before
        assert differ, f"{name}: the references of A and B are equal -- stale inputs would not show"
        self.dst = [t for t, b in inputs if b.size]
        self.b = [torch.from_numpy(np.ascontiguousarray(b)).to(t.dtype).to(sess.device) for t, b in inputs if b.size]
        assert all(d.shape == s.shape and d.dtype == s.dtype for d, s in zip(self.dst, self.b)), f"{name}: A and B differ in a size"
        self.a = [t.clone() for t in self.dst]

    def run(self, sess, between=lambda: None):
        pre = () if self.before is None else (self.before(sess),)
        between()
        return self.call(sess, *pre)

    def load(self, which):
        for d, s in zip(self.dst, which):
            d.copy_(s, non_blocking=True)


def differs(a, b):
    return any(x is not None and not np.array_equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(None)
def _recommend_host():
    """the three-class problem of the hashed cases under any + none + range and random weights; B = its queries in reverse order, so ref(B) = ref(A) reversed"""
    import recommend_hashed_cases as H
    import recommend_rules_ref as RR
    import recommend_weights_ref as W
    p = H.three_problem()
    rules = RR.make_rules(p, 5)
    wp = W.Weighted(p, W.random_weights(p, 3))
    want = W.brute_force(wp, [rules[n] for n in ("any", "none", "range")], 20)[:3]
    return p, rules, wp, want, tuple(x[::-1].copy() for x in want)


def recommend_set(sess, mp, driven):
    """call sets 1 and 2: urcco_dev_recommend_weighted under URCCO_REC_HASHED and the SMALL limits (LDS, hashed, dense), and the same under URCCO_REC_DRIVEN
    with the "any" rule's matrix as the driver (all four classes); neither synchronises"""
    import recommend_driven_cases as D
    import recommend_hashed_cases as H
    import recommend_ref as R
    import recommend_rules_ref as RR
    import recommend_weights_ref as W
    p, rules, wp, want_a, want_b = _recommend_host()
    dp = R.DeviceProblem(sess, p)
    dw = W.DeviceWeighted(dp, wp, RR.DeviceRules(dp, rules))
    dev, names = dw.dr.dev, ("any", "none", "range")
    inputs = []
    for cl, d in zip(p.clauses, dp.clauses):
        inputs += list(zip(d[4:6], rev_csr(cl.q_rp, cl.q_ci)))
    inputs += list(zip(dp.excl, rev_csr(p.excl_rp, p.excl_ci)))
    for n in ("any", "none"):
        inputs += list(zip(dev[n][4:6], rev_csr(rules[n].q_rp, rules[n].q_ci)))
    inputs += [(dev["range"][2], rules["range"].lo[::-1]), (dev["range"][3], rules["range"].hi[::-1])]
    kw, flags = {}, H.HASHED
    if driven:
        kw = dict(drivers=[(0, *D.csc(sess, rules["any"]))], clause_rows=[(R._dev(sess, cl.ind_rp), R._dev(sess, cl.ind_ci.astype(np.int32))) for cl in p.clauses])
        flags |= D.DRIVEN
    mp.setenv("URCCO_REC_DRIVE_LIMIT", str(D.SMALL))
    mp.setenv("URCCO_REC_LDS_LIMIT", str(H.SMALL[0]))
    mp.setenv("URCCO_REC_HASH_LIMIT", str(H.SMALL[1]))

    def call(s):
        return s.recommend(dp.n_queries, p.n_items, dp.clauses, 20, dp.excl, dp.mask, dp.fill, flags, rules=[dev[n] for n in names], weights=dw.dev, **kw)

    def compare(got, want):
        W.compare(got, want, "recommend")
        st = got[3]
        assert st[2] == 0 and min(st[0], st[5], st[1]) > 0 and (not driven or st[6] > 0), st      # every class served

    return CallSet("recommend driven" if driven else "recommend", sess, inputs, call, want_a, want_b, compare, differs(want_a, want_b), False)


def _audience_problem(sess):
    import audience_cases as A
    from eval_ref import put
    p = A.problem(21, 700, 6, 5)
    d_items = put(sess, p["items"])[: len(p["items"])]
    imats = [tuple(put(sess, a) for a in A.csr(ir)) for _, _, ir, _, _ in p["clauses"]]
    chunks = []
    for lo, hi in ((0, 350), (350, 700)):
        clauses = [(n, b) + im + tuple(put(sess, a) for a in A.csr(ur[lo:hi])) + (None,) for (n, b, _, ur, _), im in zip(p["clauses"], imats)]
        chunks.append((clauses, hi - lo, put(sess, p["uids"][lo:hi]), tuple(put(sess, a) for a in A.csr(p["excl"][lo:hi]))))
    return p, d_items, chunks


def _audience_compare(got, want):
    from eval_ref import bits
    count, user, score = got
    for x, (us, sc) in enumerate(want):
        k = len(us)
        assert count[x] == k and np.array_equal(user[x, :k], us) and np.array_equal(bits(score[x, :k]), bits(sc)), x
        assert (user[x, k:] == -1).all() and (score[x, k:] == 0.0).all(), x


def audience_set(sess, mp, second=False):
    """call set 4: urcco_dev_audience over two user chunks, the second accumulating into the first's result; B = the query items in reverse order.  Each
    call synchronises once, on its tile plan, so each call is a phase of its own and the delay covers what that call enqueues before its plan is read:
    `audience` puts the delay and B in front of the first chunk's call (ref(B) of both chunks), `audience_second_chunk` runs the first chunk on A, then
    puts the delay and B in front of the second chunk's call -- the reference is then the first half of the users scored against A's items merged with the
    second half scored against B's, in the order (score desc, user id asc), cut to num."""
    import audience_cases as A
    p, d_items, chunks = _audience_problem(sess)
    items_b = p["items"][::-1].copy()

    def first(s):
        *out, _ = s.audience(d_items, A.N_ITEMS, *chunks[0][:1], p["num"], *chunks[0][1:], None)
        return out

    def rest(s, out=None):
        for clauses, n, uids, excl in chunks[1:] if out is not None else chunks:
            *out, _ = s.audience(d_items, A.N_ITEMS, clauses, p["num"], n, uids, excl, out)
        return tuple(out)

    want_a, want_b = A.reference(p), A.reference(dict(p, items=items_b))
    if second:
        half = lambda lo, hi, items: A.reference(dict(p, items=items, uids=p["uids"][lo:hi], excl=p["excl"][lo:hi],      # noqa: E731
                                                      clauses=[(n, b, ir, ur[lo:hi], w) for n, b, ir, ur, w in p["clauses"]]))
        want_b = []
        for (u0, s0), (u1, s1) in zip(half(0, 350, p["items"]), half(350, 700, items_b)):
            us, sc = np.concatenate([u0, u1]), np.concatenate([s0, s1])
            order = np.lexsort((us, -sc))[: p["num"]]
            want_b.append((us[order], sc[order]))
    differ = any(not np.array_equal(a[0], b[0]) for a, b in zip(want_a, want_b))
    return CallSet("audience, second chunk" if second else "audience", sess, [(d_items, items_b)], rest, want_a, want_b, _audience_compare, differ, True,
                   before=first if second else None)


def quota_set(sess, mp):
    """call set 5: urcco_dev_quota_cut; B = the table's rows in reverse order.  The call synchronises once, on its plan: the delay covers what it enqueues
    before that."""
    import quota_cases as Q
    from eval_ref import bits, put
    p = Q.problem(*Q.CASES[12])
    n, width = p["idx"].shape
    rev = dict(p, count=p["count"][::-1].copy(), idx=p["idx"][::-1].copy(), score=p["score"][::-1].copy())
    want_a, want_b = (Q.walk(dict(q, slots=_lib.QUOTA_LDS_SLOTS))[:4] for q in (p, rev))
    count, idx, score = put(sess, p["count"]), put(sess, p["idx"]), put(sess, p["score"])
    rules = [tuple(put(sess, a) for a in Q.csr(rows)) + (m,) for rows, m in p["rules"]]

    def call(s):
        return s.quota_cut(count[:n], idx[: n * width].view(n, width), score[: n * width].view(n, width), rules, p["num"], Q.N_ITEMS)[:4]

    def compare(got, want):
        got = (got[0], got[1], bits(got[2]).reshape(got[1].shape), got[3])
        for name, g, w in zip(("count", "idx", "score", "short"), got, want):
            assert np.array_equal(g, w), name

    return CallSet("quota_cut", sess, [(count, rev["count"]), (idx, rev["idx"].reshape(-1)), (score, rev["score"].reshape(-1))], call, want_a, want_b, compare,
                   differs(want_a, want_b), True)


def append_trim_set(sess, mp, n_users=70, n_old=900, n_new=700):
    """call set 6: urcco_dev_history_append, then urcco_dev_history_trim over the index it returned, on one stream; neither synchronises.  B = the new
    events' users and the whole stream's items and times in reverse order.  The order inside a user's new index segment is unspecified, so positions are
    compared per user, sorted."""
    from eval_ref import put
    rng = np.random.default_rng(17)
    old_users = rng.integers(0, n_users, n_old).astype(np.int32)
    new_users = rng.integers(0, n_users, n_new).astype(np.int32)
    items = rng.integers(0, 1000, n_old + n_new).astype(np.int32)
    times = rng.integers(0, 100, n_old + n_new).astype(np.int64)
    drop, cut, n = np.array([3, 11, 64], np.int32), 30, n_old + n_new

    def ref(new_users, items, times):
        users = np.concatenate([old_users, new_users])
        keep = (times >= cut) & ~np.isin(users, drop)
        new_of = np.cumsum(keep) - 1
        rp = np.concatenate([[0], np.cumsum(np.bincount(users[keep], minlength=n_users))]).astype(np.int64)
        return (np.array([keep.sum(), keep.sum()], np.int64), items[keep], times[keep], rp, [np.sort(new_of[keep & (users == u)]) for u in range(n_users)],
                [np.sort(np.flatnonzero(users == u)) for u in range(n_users)])

    want_a, want_b = ref(new_users, items, times), ref(new_users[::-1], items[::-1], times[::-1])
    d_old, d_new, d_items, d_times, d_drop = (put(sess, a) for a in (old_users, new_users, items, times, drop))
    old_rp, old_pos = sess.history_index(d_old, n_users)

    def call(s):
        rp, pos = s.history_append(old_rp, old_pos, n_old, d_new, n_users)
        return (rp, pos) + tuple(s.history_trim(n, d_items, d_times, rp, pos, min_time_ms=cut, drop_users=d_drop))

    def compare(got, want):
        a_rp, a_pos, o_items, o_times, o_rp, o_pos, counts = got
        w_counts, w_items, w_times, w_rp, w_pos, w_index = want
        k = int(w_counts[0])
        assert np.array_equal(counts, w_counts) and np.array_equal(o_items[:k], w_items) and np.array_equal(o_times[:k], w_times) and np.array_equal(o_rp, w_rp)
        for u in range(n_users):
            assert np.array_equal(np.sort(a_pos[a_rp[u]:a_rp[u + 1]]), w_index[u]), ("append", u)
            assert np.array_equal(np.sort(o_pos[o_rp[u]:o_rp[u + 1]]), w_pos[u]), ("trim", u)

    differ = not np.array_equal(want_a[1], want_b[1]) and not np.array_equal(want_a[3], want_b[3])
    return CallSet("history_append + history_trim", sess, [(d_new, new_users[::-1].copy()), (d_items, items[::-1].copy()), (d_times, times[::-1].copy())], call,
                   want_a, want_b, compare, differ, False)


def chain_set(sess, mp):
    """call set 3: history_rows, recommend and explain as recommend.user_recommendations chains them, called through URAlgorithm.user_recommendations
    (explain=3, one chunk) on the handmade golden stack with a device tensor of dense user ids -- the known users, an unknown one and an id beyond the
    history, repeated; B = that tensor reversed, so ref(B) = ref(A) with its rows reversed.  ref(A) is batch_predict's answer per user (items, scores and
    "because" lists), laid out as the table.  history_rows synchronises on its bound totals (DeviceSession._bounded_rows): the delay covers the bounds
    call and the Python layer's torch ops in front of it -- the tensors of the table, the slice of the users -- and what follows runs on an idle stream.
    Its second phase cannot be given B on its own: the capacities it writes into are the totals of the inputs the first phase saw."""
    from test_recommend_rules_golden import NOW_MS, _stack
    from universal_recommender_amd.history import DeviceHistory
    algo, model, _, history, *_ = _stack(sess)
    dh = DeviceHistory.from_dict(sess, model, history)
    known = list(history)
    ids = dh.user_indices(known) + [-1, dh.n_users + 3]
    per_user = algo.batch_predict(model, [{"user": u, "num": 6} for u in known + ["nobody", "nobody"]], dh, now_ms=NOW_MS, explain=3)
    order = np.random.default_rng(5).integers(0, len(ids), 41)
    names = [("user", c.name) for c in model.correlators if c.name in dh.types]

    def table(order):
        n = len(order)
        count, idx, score = np.zeros(n, np.int32), np.full((n, 6), -1, np.int32), np.zeros((n, 6))
        w_n, w_clause, w_term, w_contrib = np.zeros((n, 6), np.int32), np.zeros((n, 6, 3), np.int32), np.zeros((n, 6, 3), np.int32), np.zeros((n, 6, 3))
        for r, k in enumerate(order):
            rows = per_user[k]["itemScores"]
            count[r] = len(rows)
            for j, row in enumerate(rows):
                idx[r, j], score[r, j], w_n[r, j] = model.item_index(row["item"]), row["score"], len(row["because"])
                for x, b in enumerate(row["because"]):
                    w_clause[r, j, x] = names.index((b["clause"], b["name"]))
                    w_term[r, j, x], w_contrib[r, j, x] = model.column_index(model.by_name[b["name"]], b["term"]), b["weight"]
        return count, idx, score.view(np.int64), w_n, w_clause, w_term, w_contrib.view(np.int64)

    want_a, want_b = table(order), table(order[::-1])
    assert int(want_a[3].sum()) > 0 and (want_a[0] > 0).any()
    users = torch.tensor([ids[k] for k in order], dtype=torch.int32).to(sess.device)

    def call(s):
        out = algo.user_recommendations(model, dh, users, num=6, now_ms=NOW_MS, explain=3)
        assert out[7] == names
        return out[:7]

    def compare(got, want):
        got = tuple(g.view(np.int64) if g.dtype == np.float64 else g for g in got)
        for name, g, w in zip(("count", "idx", "score", "n", "clause", "term", "contrib"), got, want):
            assert np.array_equal(g, w), name

    return CallSet("history_rows + recommend + explain (user_recommendations)", sess, [(users, np.array([ids[k] for k in order[::-1]], np.int32))], call,
                   want_a, want_b, compare, differs(want_a, want_b), True)


PROTOCOL = {"recommend": lambda s, mp: recommend_set(s, mp, False), "recommend_driven": lambda s, mp: recommend_set(s, mp, True), "user_recommendations": chain_set,
            "audience": audience_set, "audience_second_chunk": lambda s, mp: audience_set(s, mp, True), "quota_cut": quota_set, "append_trim": append_trim_set}


def run_protocol(cs: CallSet, sess, side, delay, log=print):
    """The steps of the protocol on the session's stream `side` (a torch stream, current): A once against ref(A) -- which leaves A's intermediates in the
    arena --, the enqueue time of the call on the idle session, then the delay, the copies of B and the call again: the bits of ref(B).  Whatever the
    library or the Python layer issued off `side` ran under the delay, on A."""
    def delay_and_b():
        delay()
        cs.load(cs.b)

    try:
        cs.compare(host(cs.run(sess)), cs.want_a)
        side.synchronize()
        t0 = time.perf_counter()
        out = cs.run(sess)
        ms = (time.perf_counter() - t0) * 1e3
        side.synchronize()
        log(f"stream contract: {cs.name}: host-side enqueue {ms:.3f} ms" + (" (synchronises by design: the time includes the wait)" if cs.syncs else ""))
        del out
        out = cs.run(sess, delay_and_b)
        idle = side.query()
        side.synchronize()
        assert cs.syncs or idle is False, f"{cs.name}: the stream was idle when the call returned -- the enqueue outlasted the delay, or the call synchronised"
        cs.compare(host(out), cs.want_b)
        return ms
    finally:
        cs.load(cs.a)
        side.synchronize()
