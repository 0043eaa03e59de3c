"""Numpy / pure-Python restatement of decision D19 (include/urcco.h urcco_dev_rank_metrics): hits, average precision and NDCG at the
cut-offs ks of a strided recommendation table against sorted truth rows, and their sums over the queries.  Written from the decision text, not from the
kernels: per-query loops in the stated order, tree() as the decision spells it.  The yardstick of tests/test_sim_eval.py and tests/test_gpu_eval.py,
which run the same checks through the helpers below (the reference's MAP@k tool lives behind Spark and Elasticsearch).

    c = min(max(count, 0), num); rel_j = rec[j] in T for j < c; H(j) = rel_0 + ... + rel_j
    hits[k] = H(min(k, c) - 1);  ap[k] = (sum_{j < min(k, c), rel_j} H(j) / (j + 1)) / min(k, |T|);  ndcg[k] = (sum ... discount[j]) / ideal[min(k, |T|)]
    every sum from 0.0 in ascending j; |T| = 0: not evaluated, outputs 0
    sums_i = [evaluated, not evaluated, sum of hits per k, queries with a hit per k];  sums_f = [tree(ap[:, k]) per k, tree(ndcg[:, k]) per k]
"""
from dataclasses import dataclass
from itertools import product
from typing import List

import numpy as np
import torch

N_ITEMS = 5000
NUMS = (1, 20, 64, 65, 256)
COUNTS = (0, 1, 63, 64, 65, 128, 255, 256, 257, 300, -2)      # the clamp on both sides: values above every num, and a negative one
TRUTH_LENS = (0, 1, 2, 63, 64, 65, 4097)
EDGES = (63, 64, 65, 127, 128, 255)                           # around the rounds of 64 positions: the carry of H
PATTERNS = ("edges", "all", "none", "last", "random")
KS_SETS = ((1,), (1, 5, 10, 20), (63, 64, 65), (1, 2, 3, 4, 5, 6, 7, 256))


def ks_sets(num):
    """the cut-off tuples of KS_SETS that fit `num`, and (num,)"""
    return list(dict.fromkeys([ks for ks in KS_SETS if ks[-1] <= num] + [(num,)]))


def discounts(num):
    """name -> position weights: the usual log2 discount, and 3^-j, whose sums change bits with the order of the adds"""
    return {"log2": 1 / np.log2(np.arange(num) + 2.0), "pow3": 3.0 ** -np.arange(num, dtype=np.float64)}


def tree(x):
    x = np.asarray(x, np.float64)
    if x.size == 0:
        return np.float64(0.0)
    size = 1
    while size < x.size:
        size *= 2
    x = np.concatenate([x, np.zeros(size - x.size, np.float64)])      # +0.0
    while x.size > 1:
        x = x[0::2] + x[1::2]
    return x[0]


def metrics_ref(num, count, idx, truth, ks, discount=None, descending=False):
    """(hits int32 [n, n_ks], ap, ndcg float64 [n, n_ks] (ndcg None without discount)); truth: per query a sorted unique int array.  descending: the
    sums in the WRONG order (the negative control of the order test)."""
    n, n_ks = len(count), len(ks)
    hits, ap = np.zeros((n, n_ks), np.int32), np.zeros((n, n_ks), np.float64)
    ndcg = np.zeros((n, n_ks), np.float64) if discount is not None else None
    ideal = [0.0]
    for j in range(num if discount is not None else 0):
        ideal.append(ideal[-1] + float(discount[j]))
    for q in range(n):
        c = min(max(int(count[q]), 0), num)
        members = set(int(i) for i in truth[q])
        t = len(members)
        if t == 0:
            continue
        rel = [int(idx[q][j]) in members for j in range(c)]
        for x, k in enumerate(ks):
            m = min(k, c)
            terms, h = [], 0
            for j in range(m):
                if rel[j]:
                    h += 1
                    terms.append((float(h) / float(j + 1), float(discount[j]) if discount is not None else 0.0))
            s = d = 0.0
            for a, b in (reversed(terms) if descending else terms):
                s = s + a
                d = d + b
            hits[q, x] = h
            ap[q, x] = s / float(min(k, t))
            if discount is not None:
                ndcg[q, x] = np.float64(d) / np.float64(ideal[min(k, t)])
    return hits, ap, ndcg


def sums_ref(truth, hits, ap, ndcg):
    n_ks = hits.shape[1]
    lens = np.array([len(r) for r in truth], np.int64)
    sums_i = np.array([np.count_nonzero(lens > 0), np.count_nonzero(lens == 0)] + [int(hits[:, x].sum()) for x in range(n_ks)] +
                      [int(np.count_nonzero(hits[:, x] > 0)) for x in range(n_ks)], np.int64)
    sums_f = np.array([tree(ap[:, x]) for x in range(n_ks)] + [tree(ndcg[:, x]) if ndcg is not None else 0.0 for x in range(n_ks)], np.float64)
    return sums_i, sums_f


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---- the planted problem ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class Problem:
    num: int
    count: np.ndarray           # int32 [n]
    idx: np.ndarray             # int32 [n, num]: every entry at or behind the clamped count is POISON, an item of the truth row
    truth: List[np.ndarray]     # sorted unique int32 per query
    plan: list                  # (count, truth length, pattern) per query

    @property
    def n(self):
        return self.count.size

    def head(self, n):
        return Problem(self.num, self.count[:n], self.idx[:n], self.truth[:n], self.plan[:n])

    def csr(self):
        rp = np.zeros(self.n + 1, np.int64)
        np.cumsum([t.size for t in self.truth], out=rp[1:])
        return rp, np.concatenate(self.truth + [np.zeros(0, np.int32)]).astype(np.int32)


def _query(rng, num, cnt, t, pattern, k_of_last):
    c = min(max(cnt, 0), num)
    truth = np.sort(rng.choice(N_ITEMS, t, replace=False)).astype(np.int32)
    others = np.setdiff1d(np.arange(N_ITEMS, dtype=np.int32), truth)
    where = {"edges": [p for p in EDGES if p < c], "all": list(range(c)), "none": [], "last": [k_of_last - 1] if k_of_last - 1 < c else [],
             "random": [int(p) for p in np.flatnonzero(rng.random(c) < 0.3)]}[pattern][:t]       # distinct entries: no more hits than truth items
    own = rng.permutation(truth)
    row = rng.choice(others, num, replace=False).astype(np.int32)
    where = np.array(where, np.int64)
    row[where] = own[: where.size]
    if t:                                                                                        # poison: a read at or behind the count shows up as a hit
        spare = own[where.size:] if where.size < t else own
        row[c:] = spare[np.arange(num - c) % spare.size]
    return row, truth


def make_problem(num, seed=0, reps=1):
    """Every count against every truth length, and every count against every hit pattern, for one table width"""
    rng = np.random.default_rng(1000 * num + seed)
    ks_last = [k for ks in ks_sets(num) for k in ks]
    plan = []
    for rep in range(reps):
        plan += [(cnt, t, PATTERNS[(i + rep) % len(PATTERNS)]) for i, (cnt, t) in enumerate(product(COUNTS, TRUTH_LENS))]
        plan += [(cnt, (4097, 64, 65)[(i + rep) % 3], pat) for i, (cnt, pat) in enumerate(product(COUNTS, PATTERNS))]
    rows, truth = [], []
    for i, (cnt, t, pat) in enumerate(plan):
        row, tr = _query(rng, num, cnt, t, pat, ks_last[i % len(ks_last)])
        rows.append(row)
        truth.append(tr)
    order = rng.permutation(len(plan))
    return Problem(num, np.array([plan[i][0] for i in order], np.int32), np.stack([rows[i] for i in order]), [truth[i] for i in order], [plan[i] for i in order])


_PROBLEMS = {}


def problem(num):
    """the shared problem of one width (built and verified once): num = 20 is the one of more than one tree block"""
    if num not in _PROBLEMS:
        p = _PROBLEMS[num] = make_problem(num, reps=2 if num == 20 else 1)
        assert_problem(p)
    return _PROBLEMS[num]


_WANT = {}


def want(num, ks, disc):
    """the restatement's answer for the shared problem, computed once and left unchanged"""
    key = (num, tuple(ks), disc)
    if key not in _WANT:
        p = problem(num)
        h, a, d = metrics_ref(num, p.count, p.idx, p.truth, ks, discounts(num)[disc] if disc else None)
        _WANT[key] = (h, a, d) + sums_ref(p.truth, h, a, d)
        for x in _WANT[key]:
            if x is not None:
                x.setflags(write=False)
    return _WANT[key]


def assert_problem(p: Problem):
    """From the restatement alone: what the generator promises.  The negative control of the order test lives here -- a descending sum changes bits
    of at least one ap and one dcg, so an implementation that adds in another order cannot pass."""
    num = p.num
    clamped = np.clip(p.count, 0, num)
    assert set(COUNTS) == set(p.count.tolist()) and (p.count > num).any() and (p.count < 0).any()
    assert {len(t) for t in p.truth} == set(TRUTH_LENS)
    for q in range(p.n):
        assert np.unique(p.idx[q, : clamped[q]]).size == clamped[q] and (np.diff(p.truth[q]) > 0).all()
        if p.truth[q].size and clamped[q] < num:
            assert np.isin(p.idx[q, clamped[q]:], p.truth[q]).all()                               # the poison
    ks = ks_sets(num)[-1] if num < 20 else (1, 5, 10, 20) if num < 65 else (63, 64, 65) if num < 256 else (1, 2, 3, 4, 5, 6, 7, 256)
    hits, ap, ndcg = metrics_ref(num, p.count, p.idx, p.truth, ks, discounts(num)["pow3"])
    by_pattern = {pat: [q for q in range(p.n) if p.plan[q][2] == pat and p.truth[q].size] for pat in PATTERNS}
    assert all(by_pattern.values())
    assert (hits[by_pattern["none"]] == 0).all()
    full = [q for q in by_pattern["all"] if p.truth[q].size >= num and clamped[q] > 0]
    assert full and all(hits[q, -1] == min(ks[-1], clamped[q]) for q in full)
    if num > 1:
        assert any(0 < p.truth[q].size < ks[-1] for q in range(p.n)) and any(p.truth[q].size > ks[-1] for q in range(p.n))   # t < k and t > k
        assert any(hits[q, -1] == 1 and hits[q, 0] == 0 for q in by_pattern["last"]) or len(ks) == 1                    # the first hit at the last position under a k
    if num >= 256:
        for q in by_pattern["edges"]:
            if clamped[q] == 256 and p.truth[q].size >= 6:
                assert hits[q].tolist() == [0] * 7 + [6]                                                               # hits at 63 / 64 / ... / 255 only
                break
        else:
            raise AssertionError("no query with hits at the round boundaries only")
    if num >= 20:
        _, ap_d, ndcg_d = metrics_ref(num, p.count, p.idx, p.truth, ks, discounts(num)["pow3"], descending=True)
        assert (bits(ap) != bits(ap_d)).any() and (bits(ndcg) != bits(ndcg_d)).any(), "the order of the sums would not show"


# ---- running it on a session -----------------------------------------------------------------------------------------------------------------------
def put(sess, a):
    a = np.ascontiguousarray(a)
    t = sess.empty(max(a.size, 1), torch.from_numpy(a.reshape(-1)[:0].copy()).dtype)      # the session's allocator: guarded under HIPSIM_GUARD
    t[: a.size].copy_(torch.from_numpy(a.reshape(-1)))
    return t


def run(sess, p: Problem, ks, discount=None, sums=True):
    """DeviceSession.rank_metrics on the problem -> numpy (hits, ap, ndcg | None, sums_i | None, sums_f | None)"""
    rp, ci = p.csr()
    out = sess.rank_metrics(put(sess, p.count)[: p.n], put(sess, p.idx)[: p.n * p.num].view(p.n, p.num), put(sess, rp), put(sess, ci), ks,
                            put(sess, discount) if discount is not None else None, sums)
    sess.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def same(got, wanted, what):
    for name, g, w in zip(("hits", "ap", "ndcg", "sums_i", "sums_f"), got, wanted):
        assert (g is None) == (w is None), (what, name)
        if g is None:
            continue
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        eq = np.array_equal(g, w) if g.dtype.kind == "i" else np.array_equal(bits(g), bits(w))
        assert eq, (what, name, np.argwhere(np.asarray(g != w))[:5].tolist() if g.shape == w.shape else None)


def check_problem(sess, num):
    """every cut-off tuple of the width under both discounts: per-query outputs and both sums equal the restatement, bit for bit"""
    p = problem(num)
    for ks in ks_sets(num):
        for disc in ("log2", "pow3"):
            got = run(sess, p, ks, discounts(num)[disc])
            same(got, want(num, ks, disc), (num, ks, disc))
    return p


def check_repeatable(sess):
    p = problem(256)
    a = run(sess, p, (1, 2, 3, 4, 5, 6, 7, 256), discounts(256)["pow3"])
    b = run(sess, p, (1, 2, 3, 4, 5, 6, 7, 256), discounts(256)["pow3"])
    same(a, b, "two runs")


def check_alignment(sess):
    """0, 1 and one more query than a block of the tree sum reduces: the padding and the pass over the partials"""
    from universal_recommender_amd import _lib
    full = problem(20)
    ks, disc = (1, 5, 10, 20), discounts(20)["pow3"]
    assert full.n > _lib.EVAL_TREE_BLOCK
    for n in (0, 1, 2, 3, _lib.EVAL_TREE_BLOCK - 1, _lib.EVAL_TREE_BLOCK, _lib.EVAL_TREE_BLOCK + 1):
        p = full.head(n)
        h, a, d = metrics_ref(20, p.count, p.idx, p.truth, ks, disc)
        got = run(sess, p, ks, disc)
        same(got, (h, a, d) + sums_ref(p.truth, h, a, d), ("n_queries", n))
        if n == 0:
            assert got[3].tolist() == [0] * 10 and got[4].tolist() == [0.0] * 8
    # the tree sum alone, over more positions than two levels of blocks reduce, against tree()
    rng = np.random.default_rng(3)
    for n in (0, 1, 255, 257, 256 * 256 + 1):
        x = 3.0 ** -rng.integers(0, 40, (n, 3)).astype(np.float64)
        got = sess.tree_sum(put(sess, x)[: n * 3].view(n, 3))
        sess.synchronize()
        assert np.array_equal(bits(got.cpu().numpy()), bits(np.array([tree(x[:, c]) for c in range(3)]))), n


def check_null_pairs(sess):
    p = problem(65)
    ks = (63, 64, 65)
    w = want(65, ks, "log2")
    same(run(sess, p, ks, discounts(65)["log2"], sums=False), w[:3] + (None, None), "no sums")
    w0 = want(65, ks, None)
    assert w0[2] is None and not w0[4][3:].any() and np.array_equal(bits(w0[1]), bits(w[1]))
    same(run(sess, p, ks, None), w0, "no discount")
    same(run(sess, p, ks, None, sums=False), w0[:3] + (None, None), "neither")


def check_bad_arguments(sess):
    """every URCCO_BAD_ARG case of include/urcco.h, through ctypes"""
    import ctypes as C
    from universal_recommender_amd import _lib
    lib = sess.lib
    p = problem(20).head(8)
    rp, ci = p.csr()
    t = {"count": put(sess, p.count), "idx": put(sess, p.idx), "rp": put(sess, rp), "ci": put(sess, ci), "disc": put(sess, discounts(20)["log2"]),
         "hits": sess.empty(8 * 8, torch.int32), "ap": sess.empty(8 * 8, torch.float64), "ndcg": sess.empty(8 * 8, torch.float64),
         "si": sess.empty(2 + 16, torch.int64), "sf": sess.empty(16, torch.float64)}

    def call(n=8, num=20, ks=(1, 5, 10, 20), n_ks=None, ks_null=False, **null):
        arr = (C.c_int32 * max(len(ks), 1))(*ks)
        a = {k: (None if null.get(k) else v.data_ptr()) for k, v in t.items()}
        return lib.urcco_dev_rank_metrics(sess.handle, n, num, a["count"], a["idx"], a["rp"], a["ci"], None if ks_null else arr, len(ks) if n_ks is None else n_ks,
                                          a["disc"], a["hits"], a["ap"], a["ndcg"], a["si"], a["sf"])

    assert call() == _lib.OK
    assert call(num=0) == _lib.BAD_ARG and call(num=_lib.REC_MAX_NUM + 1) == _lib.BAD_ARG and call(num=-5) == _lib.BAD_ARG
    assert call(ks=(), n_ks=0) == _lib.BAD_ARG and call(ks=tuple(range(1, 10))) == _lib.BAD_ARG and call(n_ks=-1) == _lib.BAD_ARG
    assert call(ks=tuple(range(1, 9))) == _lib.OK                                                   # URCCO_EVAL_MAX_KS itself
    assert call(ks=(1, 5, 5, 20)) == _lib.BAD_ARG and call(ks=(5, 1)) == _lib.BAD_ARG               # not strictly ascending
    assert call(ks=(0, 5)) == _lib.BAD_ARG and call(ks=(1, 21)) == _lib.BAD_ARG and call(ks=(-1,)) == _lib.BAD_ARG
    assert call(ks_null=True) == _lib.BAD_ARG
    assert call(n=(1 << 31) // 4) == _lib.BAD_ARG and call(n=(1 << 31), ks=(1,)) == _lib.BAD_ARG    # n_queries * n_ks >= 2^31
    assert call(n=-1) == _lib.BAD_ARG
    for name in ("count", "idx", "rp", "ci", "hits", "ap"):
        assert call(**{name: True}) == _lib.BAD_ARG, name                                           # a NULL array the call needs
    assert call(disc=True) == _lib.BAD_ARG and call(ndcg=True) == _lib.BAD_ARG and call(disc=True, ndcg=True) == _lib.OK
    assert call(si=True) == _lib.BAD_ARG and call(sf=True) == _lib.BAD_ARG and call(si=True, sf=True) == _lib.OK
    assert lib.urcco_dev_rank_metrics(None, 8, 20, *[None] * 4, (C.c_int32 * 1)(1), 1, *[None] * 6) == _lib.BAD_ARG
    assert call(n=0, count=True, idx=True, rp=True, ci=True, hits=True, ap=True, ndcg=True, disc=True) == _lib.OK   # nothing to read
    x, o = sess.empty(8, torch.float64), sess.empty(4, torch.float64)
    assert lib.urcco_dev_tree_sum(sess.handle, 2, 4, x.data_ptr(), o.data_ptr()) == _lib.OK
    for args in ((-1, 4, x.data_ptr(), o.data_ptr()), (2, 0, x.data_ptr(), o.data_ptr()), (2, 1025, x.data_ptr(), o.data_ptr()), (2, 4, None, o.data_ptr()),
                 (2, 4, x.data_ptr(), None), ((1 << 31) // 4, 4, x.data_ptr(), o.data_ptr())):
        assert lib.urcco_dev_tree_sum(sess.handle, *args) == _lib.BAD_ARG, args
    sess.synchronize()
    assert lib.urcco_version() == 305


# ---- end to end: user_recommendations and evaluate against batch_predict -----------------------------------------------------------------------------
N_USERS = 150
KS = (1, 5, 10, 20)


class Stack:
    """history_ref.predict_stack(sess, 3000, 400, 250) with the streams of history_ref.make_stream_history on the device: the training history, and test
    streams planted from the users' own batch_predict answers"""

    def __init__(self, sess):
        import history_ref as H
        from universal_recommender_amd.history import DeviceHistory
        self.sess = sess
        self.algo, self.model = H.predict_stack(sess, 3000, 400, 250)
        streams, _ = H.make_stream_history(41, N_USERS, 400, 250, max_events=60)
        self.streams = {ev: tuple(torch.from_numpy(a).to(sess.device) if a is not None else None for a in st) for ev, st in streams.items()}
        self.train = DeviceHistory.from_streams(sess, self.model, self.streams, n_users=N_USERS)
        self.idle = [u for u in range(N_USERS) if not any((st[0] == u).any() for st in streams.values())]
        assert len(self.idle) >= 2
        self.answers = self.algo.batch_predict(self.model, [{"user": u, "num": KS[-1]} for u in range(N_USERS)], self.train)
        # every third user: the items at ranks 0 and 3 of its own answer, a few random items, duplicates; the last users hold nothing
        rng = np.random.default_rng(9)
        users, items = [], []
        self.planted = [u for u in range(0, N_USERS - 10, 3)]
        for u in self.planted:
            own = [self.answers[u]["itemScores"][r]["item"] for r in (0, 3)]
            extra = [int(i) for i in rng.integers(0, 400, int(rng.integers(0, 4)))]
            mine = own + extra + own[:1] + extra[:1]
            users += [u] * len(mine)
            items += mine
        order = rng.permutation(len(users))
        self.test_users, self.test_items = np.array(users, np.int32)[order], np.array(items, np.int32)[order]
        self.test = DeviceHistory.from_streams(sess, self.model, {"purchase": (torch.from_numpy(self.test_users).to(sess.device),
                                                                                torch.from_numpy(self.test_items).to(sess.device), None)}, n_users=N_USERS)
        self.truth = [np.unique(self.test_items[self.test_users == u]) for u in range(N_USERS)]

    def table(self, answers, num):
        count = np.array([len(a["itemScores"]) for a in answers], np.int32)
        idx = np.full((len(answers), num), -1, np.int32)
        for r, a in enumerate(answers):
            idx[r, : count[r]] = [s["item"] for s in a["itemScores"]]
        return count, idx

    def report_ref(self, answers, ks=KS):
        num = ks[-1]
        count, idx = self.table(answers, num)
        hits, ap, ndcg = metrics_ref(num, count, idx, self.truth, ks, discounts(num)["log2"])
        sums_i, sums_f = sums_ref(self.truth, hits, ap, ndcg)
        ev, n_ks = int(sums_i[0]), len(ks)
        return {"ks": list(ks), "evaluated": ev, "not_evaluated": int(sums_i[1]),
                "precision": [float(int(sums_i[2 + x])) / float(ev * k) for x, k in enumerate(ks)],
                "hit_rate": [float(int(sums_i[2 + n_ks + x])) / float(ev) for x in range(n_ks)],
                "map": [float(sums_f[x]) / float(ev) for x in range(n_ks)], "ndcg": [float(sums_f[n_ks + x]) / float(ev) for x in range(n_ks)],
                "per_user": {"hits": hits, "ap": ap, "ndcg": ndcg}}


def same_report(got, wanted, what):
    for key in ("ks", "evaluated", "not_evaluated"):
        assert got[key] == wanted[key], (what, key, got[key], wanted[key])
    for key in ("precision", "hit_rate", "map", "ndcg"):
        assert np.array_equal(bits(np.array(got[key])), bits(np.array(wanted[key]))), (what, key, got[key], wanted[key])
    for key, w in wanted["per_user"].items():
        g = got["per_user"][key]
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        w = w.cpu().numpy() if torch.is_tensor(w) else w
        assert np.array_equal(g, w) if g.dtype.kind == "i" else np.array_equal(bits(g), bits(w)), (what, key)


USER_KW = ({}, {"event_names": ["view"]}, {"event_names": ["purchase"]}, {"user_bias": -1.0, "num": 5}, {"user_bias": 2.5})


def check_user_recommendations(st: Stack, on_device):
    """the table in chunks of 64 (a ragged last one) equals batch_predict's answers over the same DeviceHistory, row by row, for unknown users and users
    without events too, under every keyword set and blacklistEvents setting; the result stays on the session's device"""
    algo, model, dh = st.algo, st.model, st.train
    users = list(range(N_USERS)) + [-1, N_USERS, N_USERS + 7]
    assert set(st.idle) <= set(users)
    positive = False
    try:
        for blacklist in (None, [], ["purchase", "view"]):
            algo.ap.blacklistEvents = blacklist
            for kw in USER_KW:
                q_kw = {k2: kw[k] for k, k2 in (("num", "num"), ("event_names", "eventNames"), ("user_bias", "userBias")) if k in kw}
                wanted = algo.batch_predict(model, [dict(q_kw, user=u) for u in users], dh)
                count, idx, score = algo.user_recommendations(model, dh, users, chunk=64, **kw)
                assert count.device == idx.device == score.device == st.sess.device and on_device == count.is_cuda
                num = kw.get("num", 10)
                assert idx.shape == (len(users), num) and score.shape == idx.shape and idx.dtype == torch.int32 and score.dtype == torch.float64
                count, idx, score = count.cpu().numpy(), idx.cpu().numpy(), score.cpu().numpy()
                for r, w in enumerate(wanted):
                    assert [{"item": int(idx[r, j]), "score": float(score[r, j])} for j in range(int(count[r]))] == w["itemScores"], (blacklist, kw, users[r])
                    assert (idx[r, count[r]:] == -1).all() and (score[r, count[r]:] == 0.0).all()
                positive |= any(s["score"] > 0 for r in wanted for s in r["itemScores"])
                by_id = algo.user_recommendations(model, dh, torch.tensor(users, dtype=torch.int32).to(st.sess.device), chunk=100, **kw)
                assert np.array_equal(by_id[1].cpu().numpy(), idx) and np.array_equal(bits(by_id[2].cpu().numpy()), bits(score))
    finally:
        algo.ap.blacklistEvents = None
    assert positive
    whole = algo.user_recommendations(model, dh)
    part = algo.user_recommendations(model, dh, torch.arange(N_USERS, dtype=torch.int32, device=st.sess.device), chunk=64)
    assert all(torch.equal(a, b) for a, b in zip(whole, part)) and whole[0].numel() == N_USERS


def check_user_recommendations_errors(st: Stack):
    import pytest
    algo, model, dh = st.algo, st.model, st.train
    with pytest.raises(ValueError):
        algo.user_recommendations(model, {0: {"purchase": [1]}})
    for bad in ({"num": 0}, {"num": 257}, {"chunk": 0}, {"users": torch.zeros(3, dtype=torch.int64)}, {"users": torch.zeros((2, 2), dtype=torch.int32)}):
        with pytest.raises(ValueError):
            algo.user_recommendations(model, dh, **bad)
    props, model.properties = model.properties, None
    try:
        with pytest.raises(NotImplementedError):
            algo.user_recommendations(model, dh, user_bias=-1.0)
    finally:
        model.properties = props


def check_evaluate(st: Stack):
    import pytest
    from universal_recommender_amd import evaluate as E
    from universal_recommender_amd.history import DeviceHistory, _Stream
    algo, model = st.algo, st.model
    wanted = st.report_ref(st.answers)
    planted = [u for u in st.planted if (st.truth[u] >= 0).any()]
    assert wanted["evaluated"] == len(planted) == len(st.planted) and wanted["not_evaluated"] == N_USERS - len(planted) >= 10
    assert wanted["hit_rate"][-1] == 1.0 and wanted["hit_rate"][0] == 1.0 and 0 < wanted["map"][-1] < 1 and 0 < wanted["ndcg"][-1] < 1      # hits by construction
    reports = {chunk: algo.evaluate(model, st.train, st.test, ks=KS, chunk=chunk) for chunk in (64, 100, 65536)}
    for chunk, got in reports.items():
        same_report(got, wanted, chunk)
        assert all(torch.is_tensor(t) and t.device == st.sess.device and t.shape == (N_USERS, len(KS)) for t in got["per_user"].values())
    same_report(reports[64], reports[65536], "chunk")
    # a wider table than the largest cut-off, other cut-offs
    same_report(algo.evaluate(model, st.train, st.test, ks=(3, 10), chunk=64),
                st.report_ref(algo.batch_predict(model, [{"user": u, "num": 10} for u in range(N_USERS)], st.train), (3, 10)), "ks")
    # two event mixes: two reports that differ, each the report of its mix
    mixes = [["purchase"], ["view"]]
    two = algo.evaluate(model, st.train, st.test, ks=KS, event_names=mixes, chunk=100)
    assert isinstance(two, list) and len(two) == 2
    for mix, got in zip(mixes, two):
        same_report(got, st.report_ref(algo.batch_predict(model, [{"user": u, "num": KS[-1], "eventNames": mix} for u in range(N_USERS)], st.train)), mix)
    assert two[0]["map"] != two[1]["map"] and not torch.equal(two[0]["per_user"]["ap"], two[1]["per_user"]["ap"])
    # nobody evaluated: zeros, not a division by zero
    empty = DeviceHistory.from_streams(st.sess, model, {"purchase": (torch.zeros(0, dtype=torch.int32, device=st.sess.device),) * 2 + (None,)}, n_users=N_USERS)
    got = algo.evaluate(model, st.train, empty, ks=(1, 5))
    assert got["evaluated"] == 0 and got["not_evaluated"] == N_USERS and got["map"] == got["ndcg"] == got["precision"] == got["hit_rate"] == [0.0, 0.0]
    # ValueErrors
    other = DeviceHistory.from_streams(st.sess, model, {"purchase": st.streams["purchase"]}, n_users=N_USERS + 1)
    s = st.test.types["purchase"]
    mapped = DeviceHistory(st.sess, N_USERS, None, {"purchase": _Stream(s.n_cols, s.idx_row_ptr, s.idx_pos, s.items, s.times, torch.zeros(s.n_cols, dtype=torch.int32, device=st.sess.device))})
    for bad in (lambda: algo.evaluate(model, st.train, {}), lambda: algo.evaluate(model, {}, st.test), lambda: algo.evaluate(model, st.train, other),
                lambda: algo.evaluate(model, st.train, mapped), lambda: algo.evaluate(model, st.train, st.test, truth_event="view"),
                lambda: algo.evaluate(model, st.train, st.test, ks=(5, 1)), lambda: algo.evaluate(model, st.train, st.test, ks=()),
                lambda: algo.evaluate(model, st.train, st.test, ks=(1, 5), num=4), lambda: algo.evaluate(model, st.train, st.test, ks=tuple(range(1, 10)))):
        with pytest.raises(ValueError):
            bad()
    # split_streams: the two halves are the stream, every time of the first is < at_ms; a stream without times cannot be split
    users, items, times = st.streams["purchase"]
    at = int(times.median())
    before, later = E.split_streams({"purchase": st.streams["purchase"]}, at)
    (bu, bi, bt), (lu, li, lt) = before["purchase"], later["purchase"]
    assert 0 < bt.numel() < times.numel() and bool((bt < at).all()) and bool((lt >= at).all()) and bt.numel() + lt.numel() == times.numel()
    early = (times < at).cpu().numpy()
    for whole, a, b in ((users, bu, lu), (items, bi, li), (times, bt, lt)):
        w = whole.cpu().numpy()
        assert np.array_equal(a.cpu().numpy(), w[early]) and np.array_equal(b.cpu().numpy(), w[~early]) and a.device == whole.device
    with pytest.raises(ValueError):
        E.split_streams(st.streams, at)                                                             # "view" has no times
