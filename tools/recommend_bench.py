#!/usr/bin/env python3
"""Times urcco_dev_recommend (HIP events, warm, several repetitions) against the same result computed with PyTorch-ROCm plumbing on the same
GPU: a chunked torch.sparse product per clause into a dense (queries x items) chunk, exclusions struck out, torch.topk.

Shapes: a model of 200K items and 5 event types with k = 50 (BASELINE config 4's event mix at a tenth of its item spaces, built on the device
by this library), 100K user queries whose histories are the users' own rows of the event matrices (lengths as synth.py draws them), the
user's primary-event items as the blacklist, popularity as the backfill order, num = 20.
--rules: the same problem once more through urcco_dev_recommend_rules under one category filter (an ANY rule on a value that about half of the
catalogue holds) and one NONE rule (a value a ninth of it holds), its time printed next to the rule-free call's; the first measurement of that
path belongs under profiles/ (DESIGN.md section 7a).
--device-history: the event-store half of the same queries (decision D17).  The event matrices are unrolled into (user, item, time) streams on the
device, indexed (urcco_dev_history_index), and the queries' term rows and exclusion rows built by urcco_dev_history_bounds + _rows (caps 500, the
primary as the blacklist event); their device time (HIP events, the read of the bound totals in between included) is printed next to the wall time
of the host planning of recommend.batch_predict's dict form for the same queries (per query and event type: reversed slice, dict.fromkeys, one
dictionary lookup per item, np.unique) on this box.
--device-items: the model half of --queries item queries (decision D18), one per item from item 0 on (wrapping around the catalogue): the device time
(HIP events, the read of the bound totals included) of urcco_dev_item_bounds + _rows over the model's indicator matrices, next to the wall time of the
host planning recommend.batch_predict does for the same queries on this box -- the one-off copy of every indicator matrix to the host, printed on
its own, then per query and event type a slice, an astype and np.unique, and the CSR of the rows.  --no-torch skips the torch comparison.
--evaluate: hold-out evaluation of the model (decision D19) for the --queries users.  The training history is the users' rows of the event matrices as
streams on the device; the held-out events are one more draw of the primary event by synth.py (same popularity, user ids beyond the trained ones, taken
as the first --queries users').  Printed: the HIP-event time of urcco_dev_rank_metrics alone (ks = 1, 5, 10, 20, the sums included) over a table and truth
rows built beforehand; the wall time of URAlgorithm.evaluate end to end (user_recommendations + truth rows + rank_metrics per chunk, the tree sums, one
report); and, as a comparison point only, the HIP-event time of a torch.isin + cumsum restatement of the per-user hits on the same GPU.
--weights: the same problem once more through urcco_dev_recommend_weighted (decision D20) under the model's idf term weights (DeviceModel.term_weights:
one urcco_dev_idf_weights call per event type, timed on its own), its time printed next to the unweighted call's of the same process; and once with arrays
that hold WEIGHT_ONE alone, whose ids and score bits must be the unweighted call's.
usage: tools/recommend_bench.py [--users N] [--queries N] [--chunk N] [--reps N] [--rules] [--weights] [--device-history] [--device-items] [--evaluate] [--no-torch]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from universal_recommender_amd import _lib, synth  # noqa: E402
from universal_recommender_amd.device import DatasetParams, DevCsr, DeviceSession, cross_occurrence_device  # noqa: E402
from universal_recommender_amd.recommend import DeviceModel, _csr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=1_000_000)
ap.add_argument("--queries", type=int, default=100_000)
ap.add_argument("--chunk", type=int, default=2048)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--num", type=int, default=20)
ap.add_argument("--rules", action="store_true", help="also time the call under an ANY and a NONE rule")
ap.add_argument("--weights", action="store_true", help="also time the weighted call under idf term weights")
ap.add_argument("--device-history", action="store_true", help="also time history_bounds + history_rows against the host planning loop")
ap.add_argument("--device-items", action="store_true", help="also time item_bounds + item_rows against the host planning loop of item queries")
ap.add_argument("--evaluate", action="store_true", help="also time rank_metrics, evaluate end to end and a torch restatement of the hits")
ap.add_argument("--no-torch", action="store_true", help="skip the torch comparison")
args = ap.parse_args()

assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
dev = torch.device("cuda", 0)
cfg = synth.config4(args.users / 10_000_000, item_scale=0.1)
mats = [DevCsr(cfg.n_users, nc, rp, ci, int(rp[-1].item())) for (_, nc, rp, ci) in synth.generate_device(cfg, dev)]
sess = DeviceSession(dev, _lib.load(os.environ.get("URCCO_LIB", _lib.DEFAULT_PATH)))
K = 50
inds = cross_occurrence_device(sess, mats, [DatasetParams(500, K, None) for _ in mats], 1)
sess.synchronize()
names = [e.name for e in cfg.events]
model = DeviceModel.from_indicators(sess, list(zip(names, inds)))
n_items, nq, num = model.n_items, min(args.queries, cfg.n_users), args.num
pop = torch.bincount(mats[0].col_idx[: mats[0].nnz_bound].to(torch.int64), minlength=n_items)
fill = torch.sort(-pop, stable=True).indices.to(torch.int32)
boosts = [1.0, 1.05, 2.0, 0.5, 20.0][: len(mats)]
clauses, lens = [], []
for c, m, b in zip(model.correlators, mats, boosts):
    qrp = m.row_ptr[: nq + 1].contiguous()
    clauses.append((c.n_cols, b, c.col_ptr, c.row_idx, qrp, m.col_idx))
    lens.append(float(qrp[-1].item()) / nq)
excl = (mats[0].row_ptr[: nq + 1].contiguous(), mats[0].col_idx)
print(f"model: {n_items} items, {len(mats)} event types {[c.n_cols for c in model.correlators]}, k = {K}, indicator entries {[int(c.row_ptr[-1].item()) for c in model.correlators]}")
print(f"queries: {nq} users, mean history length per event {[round(x, 1) for x in lens]}, num = {num}")


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, ms


(count, idx, score, stats), ms_hip = timed(lambda: sess.recommend(nq, n_items, clauses, num, excl, None, fill, 0), args.reps)
st = stats.cpu().tolist()
print(f"urcco_dev_recommend: {min(ms_hip):.2f} ms best, {sorted(ms_hip)[len(ms_hip) // 2]:.2f} ms median of {args.reps} ({[round(x, 2) for x in ms_hip]})")
print(f"  class split: {st[0]} queries in the LDS class, {st[1]} in the global class; table overflows {st[2]}; candidates {st[3]} ({st[3] / nq:.0f} per query)")

if args.rules:
    # item x value matrix of 10 values: value 0 on every second item (the filter), value 1 + i % 9 on every item (the NONE rule names value 1)
    g = torch.Generator(device="cpu").manual_seed(1)
    half = (torch.rand(n_items, generator=g) < 0.5).to(dev)
    item = torch.arange(n_items, device=dev)
    m_rp = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(1 + half.to(torch.int64), 0)])
    m_ci = torch.empty(int(m_rp[-1].item()), dtype=torch.int32, device=dev)
    m_ci[m_rp[:-1]] = (1 + item % 9).to(torch.int32)
    m_ci[m_rp[1:][half] - 1] = 0
    one = torch.arange(nq + 1, dtype=torch.int64, device=dev)   # every query row holds one value
    rules = [(_lib.RULE_ANY, 10, m_rp, m_ci, one, torch.zeros(nq, dtype=torch.int32, device=dev)),
             (_lib.RULE_NONE, 10, m_rp, m_ci, one, torch.ones(nq, dtype=torch.int32, device=dev))]
    (r_count, _, _, r_stats), ms_rules = timed(lambda: sess.recommend(nq, n_items, clauses, num, excl, None, fill, 0, rules=rules), args.reps)
    rs = r_stats.cpu().tolist()
    print(f"urcco_dev_recommend_rules (ANY on a value {float(half.float().mean()):.0%} of the items hold, NONE on a value a ninth hold): {min(ms_rules):.2f} ms best, "
          f"{sorted(ms_rules)[len(ms_rules) // 2]:.2f} ms median of {args.reps} ({[round(x, 2) for x in ms_rules]}) -- rule-free call above: {min(ms_hip):.2f} ms")
    print(f"  candidates {rs[3]} ({rs[3] / nq:.0f} per query, {st[3] / nq:.0f} without rules); backfill steps {rs[4]} ({rs[4] / nq:.2f} per query); full rows {int((r_count == num).sum())} / {nq}")

if args.weights:
    _, ms_idf = timed(lambda: [sess.idf_weights(c.col_ptr, c.n_cols, n_items) for c in model.correlators], args.reps)
    tw = model.term_weights("idf")
    w_idf = [tw[c.name] for c in model.correlators]
    (w_count, w_idx, w_score, w_stats), ms_w = timed(lambda: sess.recommend(nq, n_items, clauses, num, excl, None, fill, 0, weights=w_idf), args.reps)
    ws = w_stats.cpu().tolist()
    print(f"urcco_dev_idf_weights, {len(w_idf)} calls over {[c.n_cols for c in model.correlators]} columns: {min(ms_idf):.3f} ms best ({[round(x, 3) for x in ms_idf]}); "
          f"weights per event type (min, max, in units of 2^-15): {[(int(w.view(torch.int32).min().item()), int(w.view(torch.int32).max().item())) for w in w_idf]}")
    print(f"urcco_dev_recommend_weighted (idf weights on every clause): {min(ms_w):.2f} ms best, {sorted(ms_w)[len(ms_w) // 2]:.2f} ms median of {args.reps} "
          f"({[round(x, 2) for x in ms_w]}) -- unweighted call above: {min(ms_hip):.2f} ms best, {sorted(ms_hip)[len(ms_hip) // 2]:.2f} ms median")
    live = torch.arange(num, device=dev)[None, :] < count[:, None]
    moved = ((w_idx != idx) & live).any(1)
    print(f"  class split: {ws[0]} LDS, {ws[1]} global; candidates {ws[3]} (unweighted {st[3]}); counts equal: {bool(torch.equal(w_count, count))}; "
          f"queries whose list differs from the unweighted one: {int(moved.sum())} / {nq}")
    ones = [torch.full((c.n_cols,), _lib.REC_WEIGHT_ONE, dtype=torch.int32, device=dev).view(torch.uint32) for c in model.correlators]
    o_count, o_idx, o_score, _ = sess.recommend(nq, n_items, clauses, num, excl, None, fill, 0, weights=ones)
    print(f"  arrays of WEIGHT_ONE: counts, ids and score bits equal the unweighted call's: "
          f"{bool(torch.equal(o_count, count) and torch.equal(torch.where(live, o_idx, 0), torch.where(live, idx, 0)) and torch.equal(torch.where(live, o_score, 0.0).view(torch.int64), torch.where(live, score, 0.0).view(torch.int64)))}")

if args.device_history:
    import time

    import numpy as np
    CAP = 500
    g = torch.Generator(device="cpu").manual_seed(2)
    streams, host = [], []
    for m in mats:
        nnz = m.nnz_bound
        users = torch.repeat_interleave(torch.arange(m.n_rows, device=dev, dtype=torch.int32), (m.row_ptr[1:] - m.row_ptr[:-1]))
        perm = torch.randperm(nnz, generator=g).to(dev)                   # an event stream is not sorted by user
        users, items = users[perm].contiguous(), m.col_idx[:nnz][perm].contiguous()
        times = (1_600_000_000_000 + torch.randint(0, 30 * 86_400_000, (nnz,), generator=g)).to(dev)
        rp, pos = sess.history_index(users, m.n_rows)
        streams.append((m.n_cols, rp, pos, items, times))
    specs = [(nc, CAP, t == 0, rp, pos, items, times, None) for t, (nc, rp, pos, items, times) in enumerate(streams)]
    q_users = torch.arange(nq, dtype=torch.int32, device=dev)
    ms_hist = []
    for r in range(args.reps + 1):
        rows, ex, info = sess.history_rows(q_users, cfg.n_users, specs, n_items, None, stats=True, timing=True)
        if r:
            ms_hist.append(info["ms"])
    hs = info["stats"].cpu().tolist()
    print(f"urcco_dev_history_bounds + _rows ({nq} queries x {len(mats)} event types, cap {CAP}): {min(ms_hist):.2f} ms best, {sorted(ms_hist)[len(ms_hist) // 2]:.2f} ms median "
          f"of {args.reps} ({[round(x, 2) for x in ms_hist]})")
    print(f"  pairs by class: wave {hs[0]}, block {hs[1]}, global {hs[2]}; ran the select {hs[3]}; exclusion rows: wave {hs[4]}, block {hs[5]}; term entries "
          f"{[int(rp[-1].item()) for rp, _ in rows]}, exclusion entries {int(ex[0][-1].item())}")
    # the host planning of the dict form for the same queries: the history as Python lists (built outside the timed part), ids through a dict per event type
    h_rows = [(m.row_ptr[: nq + 1].cpu().numpy(), m.col_idx[: int(m.row_ptr[nq].item())].cpu().numpy()) for m in mats]
    lists = [[[str(i) for i in ci[rp[u]:rp[u + 1]]] for u in range(nq)] for rp, ci in h_rows]
    dicts = [{str(i): i for i in range(m.n_cols)} for m in mats]
    t0 = time.perf_counter()
    for u in range(nq):
        for t in range(len(mats)):
            recent = list(reversed(lists[t][u]))[:CAP]
            ids = [dicts[t].get(i) for i in dict.fromkeys(recent)]
            np.unique(np.array([i for i in ids if i is not None], np.int64))
        np.unique(np.array([dicts[0].get(i) for i in lists[0][u]], np.int64))
    host_ms = (time.perf_counter() - t0) * 1e3
    print(f"host planning loop of the dict form, same queries (recommend.py, one thread): {host_ms:.0f} ms wall -- {host_ms / min(ms_hist):.0f}x the device calls")

if args.device_items:
    import time

    import numpy as np
    MQE = 5000                                                            # maxQueryEvents of five indicators at the default maxItemsPerUser: nothing is cut at k = 50
    nqi = args.queries
    q_items = (torch.arange(nqi, device=dev) % n_items).to(torch.int32)
    specs = [(c.n_cols, MQE, c.row_ptr, c.col_idx) for c in model.correlators]
    ms_items = []
    for r in range(args.reps + 1):
        rows, info = sess.item_rows(q_items, specs, stats=True, timing=True, n_items=n_items)
        if r:
            ms_items.append(info["ms"])
    its = info["stats"].cpu().tolist()
    print(f"urcco_dev_item_bounds + _rows ({nqi} item queries x {len(specs)} event types, maxQueryEvents {MQE}): {min(ms_items):.2f} ms best, "
          f"{sorted(ms_items)[len(ms_items) // 2]:.2f} ms median of {args.reps} ({[round(x, 2) for x in ms_items]})")
    print(f"  pairs by class: wave {its[0]}, block {its[1]}, global {its[2]}; cut {its[3]}; term entries {[int(rp[-1].item()) for rp, _ in rows]}")
    # the host planning of recommend.batch_predict for the same queries: DeviceModel.indicator_row's copy of the matrices, then the per-query loop
    for c in model.correlators:
        c.host = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for c in model.correlators:
        model.indicator_row(c, 0)
    copy_ms = (time.perf_counter() - t0) * 1e3
    q_host = q_items.cpu().tolist()
    t0 = time.perf_counter()
    planned = [[] for _ in model.correlators]
    for i in q_host:
        for t, c in enumerate(model.correlators):
            ids = model.indicator_row(c, i)
            if ids.size > MQE:
                ids = ids[: MQE - 1]
            planned[t].append(np.unique(ids.astype(np.int64)))
    for p_rows in planned:                                                # the clause rows of the call, as batch_predict ships them
        _csr(p_rows, dev)
    torch.cuda.synchronize()
    loop_ms = (time.perf_counter() - t0) * 1e3
    print(f"host planning of the same item queries (recommend.py, one thread): matrices to the host once {copy_ms:.0f} ms wall, per-query loop {loop_ms:.0f} ms wall")

if args.evaluate:
    import dataclasses
    import time

    from universal_recommender_amd.evaluate import TRUTH_CAP, log2_discount
    from universal_recommender_amd.history import DeviceHistory
    from universal_recommender_amd.ur_algorithm import URAlgorithm, URAlgorithmParams
    KS = (1, 5, 10, 20)
    engine = {"algorithms": [{"name": "ur", "params": {"appName": "bench", "indexName": "bench", "typeName": "items", "num": num,
                                                       "indicators": [{"name": n} for n in names]}}]}
    algo = URAlgorithm(URAlgorithmParams.from_engine_json(engine), device=0, library=sess.lib)

    def stream(rp, ci):          # the first nq rows of a CSR as (user, item) events
        users = torch.repeat_interleave(torch.arange(nq, device=dev, dtype=torch.int32), rp[1: nq + 1] - rp[:nq])
        return users, ci[: int(rp[nq].item())].contiguous(), None

    train = DeviceHistory.from_streams(sess, model, {n: stream(m.row_ptr, m.col_idx) for n, m in zip(names, mats)}, n_users=nq)
    _, _, h_rp, h_ci = synth.generate_device(dataclasses.replace(cfg, events=cfg.events[:1]), dev, user_lo=cfg.n_users, user_hi=cfg.n_users + nq)[0]
    test = DeviceHistory.from_streams(sess, model, {names[0]: stream(h_rp, h_ci)}, n_users=nq)
    q_users = torch.arange(nq, dtype=torch.int32, device=dev)
    u_count, u_idx, _ = algo.user_recommendations(model, train, q_users, num)
    ts = test.types[names[0]]
    (truth,), _, _ = sess.history_rows(q_users, nq, [(ts.n_cols, TRUTH_CAP, False, ts.idx_row_ptr, ts.idx_pos, ts.items, ts.times, None)], n_items)
    disc = torch.from_numpy(log2_discount(num)).to(dev)
    (e_hits, _, _, e_si, _), ms_rank = timed(lambda: sess.rank_metrics(u_count, u_idx, truth[0], truth[1], KS, disc), args.reps)
    si = e_si.cpu().tolist()
    print(f"urcco_dev_rank_metrics ({nq} users, num = {num}, ks = {list(KS)}, {int(truth[0][-1].item())} truth entries, sums included): {min(ms_rank):.3f} ms best, "
          f"{sorted(ms_rank)[len(ms_rank) // 2]:.3f} ms median of {args.reps} ({[round(x, 3) for x in ms_rank]})")
    print(f"  evaluated {si[0]}, not evaluated {si[1]}, hits per k {si[2:2 + len(KS)]}, users with a hit per k {si[2 + len(KS):]}")
    algo.evaluate(model, train, test, ks=KS, num=num)                       # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    report = algo.evaluate(model, train, test, ks=KS, num=num)
    torch.cuda.synchronize()
    print(f"URAlgorithm.evaluate end to end, second call ({nq} users, chunk 65536): {(time.perf_counter() - t0) * 1e3:.1f} ms wall")
    print(f"  precision {[round(x, 5) for x in report['precision']]}, hit rate {[round(x, 5) for x in report['hit_rate']]}, "
          f"MAP {[round(x, 5) for x in report['map']]}, NDCG {[round(x, 5) for x in report['ndcg']]}")
    ks_t = torch.tensor(KS, device=dev) - 1

    def torch_hits():            # membership of (row, item) keys, then a running count along the row
        live = torch.arange(num, device=dev)[None, :] < u_count[:, None]
        rec_key = torch.arange(nq, device=dev)[:, None] * n_items + u_idx.to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(nq, device=dev), truth[0][1:] - truth[0][:-1])
        truth_key = rows * n_items + truth[1][: rows.numel()].to(torch.int64)
        rel = torch.isin(rec_key, truth_key) & live
        return rel.cumsum(1)[:, ks_t].to(torch.int32)

    t_hits, ms_isin = timed(torch_hits, args.reps)
    print(f"torch.isin + cumsum restatement of the per-user hits alone (comparison point): {min(ms_isin):.3f} ms best ({[round(x, 3) for x in ms_isin]}); "
          f"hits equal: {bool(torch.equal(t_hits, e_hits))}")

if args.no_torch:
    sess.close()
    sys.exit(0)

# ---- the same with torch: per chunk of queries, sum_c boost_c * T_c[chunk] @ I_c' (sparse x sparse -> dense), key = score with the backfill position as tie break ----
pos = torch.empty(n_items, dtype=torch.int64, device=dev)
pos[fill.to(torch.int64)] = torch.arange(n_items, device=dev)
tie = pos.to(torch.float64) * 1e-9   # scores are sums of boost * integer: gaps of >= 0.05 against at most 2e-4 of tie break
ind_t = []
for c in model.correlators:
    nnz = int(c.row_ptr[-1].item())
    i_csr = torch.sparse_csr_tensor(c.row_ptr, c.col_idx[:nnz].to(torch.int64), torch.ones(nnz, dtype=torch.float64, device=dev), size=(n_items, c.n_cols))
    ind_t.append(i_csr.to_sparse_coo().t().coalesce())     # (n_cols x n_items)
mode = {"name": "sparse x sparse"}


def torch_path():
    out_idx = torch.empty((nq, num), dtype=torch.int64, device=dev)
    out_score = torch.empty((nq, num), dtype=torch.float64, device=dev)
    for lo in range(0, nq, args.chunk):
        hi = min(lo + args.chunk, nq)
        dense = torch.zeros((hi - lo, n_items), dtype=torch.float64, device=dev)
        for (n_cols, b, _, _, qrp, qci), it in zip(clauses, ind_t):
            s, e = int(qrp[lo].item()), int(qrp[hi].item())
            rows = torch.repeat_interleave(torch.arange(hi - lo, device=dev), (qrp[lo + 1: hi + 1] - qrp[lo: hi]))
            t = torch.sparse_coo_tensor(torch.stack([rows, qci[s:e].to(torch.int64)]), torch.ones(e - s, dtype=torch.float64, device=dev), size=(hi - lo, n_cols)).coalesce()
            if mode["name"] == "sparse x sparse":
                dense += b * torch.sparse.mm(t, it).to_dense()
            else:
                dense += b * torch.sparse.mm(it.t(), t.to_dense().t()).t()
        key = dense - tie
        s, e = int(excl[0][lo].item()), int(excl[0][hi].item())
        rows = torch.repeat_interleave(torch.arange(hi - lo, device=dev), (excl[0][lo + 1: hi + 1] - excl[0][lo: hi]))
        key[rows, excl[1][s:e].to(torch.int64)] = float("-inf")
        top = torch.topk(key, num, dim=1)
        out_idx[lo:hi] = top.indices
        out_score[lo:hi] = torch.gather(dense, 1, top.indices)
    return out_idx, out_score


try:
    (t_idx, t_score), ms_torch = timed(torch_path, max(args.reps // 2, 1), warm=1)
except RuntimeError as err:
    print(f"  (torch: sparse x sparse product not available here: {str(err)[:120]}; using sparse x dense)")
    mode["name"] = "sparse x dense"
    (t_idx, t_score), ms_torch = timed(torch_path, max(args.reps // 2, 1), warm=1)
print(f"torch ({mode['name']}, chunks of {args.chunk} queries, topk): {min(ms_torch):.2f} ms best ({[round(x, 2) for x in ms_torch]})")
full = count.to(torch.int64) == num
same_ids = (idx.to(torch.int64) == t_idx).all(1) | ~full
same_scores = (score == t_score).all(1) | ~full
print(f"agreement on the {int(full.sum())} full rows: ids {int(same_ids.sum())} / {nq}, scores {int(same_scores.sum())} / {nq}")
print(f"ratio torch / hand-written: {min(ms_torch) / min(ms_hip):.2f}x")
sess.close()
