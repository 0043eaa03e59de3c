"""Hold-out evaluation of a built model on the GPU that holds it: MAP@k, NDCG@k, precision and hit rate over the users of a test history
(decision D19 of DESIGN.md; include/urcco.h urcco_dev_rank_metrics).

The reference leaves this to its MAP@k tool, for which its query key `eventNames` exists ("for indicator predictiveness testing",
URAlgorithm.scala:401 `queryEventNames`): train on the events before a split, ask for every user's recommendations under an event mix, and score
them against what the user did afterwards.  Here the users' recommendations come from recommend.user_recommendations over the training
history, the held-out sets are the test history's term rows of the truth event (decision D17, cap 2^31 - 1: every event), and
urcco_dev_rank_metrics scores `chunk` users per call.  The per-user values of all chunks land in one [n_users, n_ks] tensor per metric and
urcco_dev_tree_sum adds each column once, in the fixed pairwise order of the decision: the report does not depend on `chunk`, and every number
in it is reproducible bit for bit.

list_metrics (decision D35) judges what a table SHOWS rather than whether it is right: catalogue coverage, the Gini coefficient and the Herfindahl index
of the exposure, novelty and intra-list similarity, from the exact integers of urcco_dev_list_exposure / _exposure_stats / _list_links."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .history import DeviceHistory
from .recommend import DeviceModel, user_recommendations

TRUTH_CAP = 2**31 - 1     # max_items of the truth rows: n_u <= max_items skips the select (D17)


def log2_discount(num: int) -> np.ndarray:
    """The position weights of the usual NDCG, 1 / log2(j + 2) for j < num, evaluated here on the host: the kernel never takes a logarithm"""
    return 1 / np.log2(np.arange(num) + 2.0)


def _report(ks, sums_i, tree_ap, tree_ndcg, per_user) -> dict:
    n_ks = len(ks)
    evaluated, skipped = int(sums_i[0]), int(sums_i[1])
    over = (lambda v: float(v) / float(evaluated)) if evaluated else (lambda v: 0.0)
    return {"ks": list(ks), "evaluated": evaluated, "not_evaluated": skipped,
            "precision": [float(int(sums_i[2 + x])) / float(evaluated * k) if evaluated else 0.0 for x, k in enumerate(ks)],
            "hit_rate": [over(int(sums_i[2 + n_ks + x])) for x in range(n_ks)],
            "map": [over(tree_ap[x]) for x in range(n_ks)],
            "ndcg": [over(tree_ndcg[x]) for x in range(n_ks)],
            "per_user": per_user}


def self_information(popularity, n_items: int):
    """(info, seen): info[i] = -log2(pop[i] / sum of pop) for the novelty of list_metrics where seen[i] = pop[i] > 0, else 0.0 -- evaluated here on the
    host, like log2_discount.  popularity: a per-item count (tensor or array, n_items entries), e.g. the `popular` rank counts of DeviceHistory.ranks."""
    pop = np.asarray(popularity.cpu() if torch.is_tensor(popularity) else popularity).astype(np.int64).reshape(-1)
    if pop.size != n_items:
        raise ValueError(f"popularity: one count per item expected, got {pop.size} for {n_items} items")
    pop = np.where(pop > 0, pop, 0)
    info = np.zeros(n_items, np.float64)
    seen = pop > 0
    info[seen] = -np.log2(pop[seen].astype(np.float64) / np.float64(int(pop.sum())))
    return info, seen


def _list_chunk(model: DeviceModel, count, idx, ks, bucket, linked_out):
    """one chunk of a table into the histogram and into its rows of `linked`"""
    sess, sim = model.sess, model.correlators[0]
    bucket = sess.list_exposure(count, idx, ks, model.n_items, bucket)
    sess.list_links(count, idx, sim.row_ptr, sim.col_idx, ks, model.n_items, out=linked_out)
    return bucket


def _list_report(model: DeviceModel, ks, bucket, count, linked, popularity) -> dict:
    """The floats of decision D35 from the kernels' integers: Python ints for coverage, gini and herfindahl; one f64 division per row and one
    urcco_dev_tree_sum per metric for ils and novelty.  Synchronises."""
    sess, dev, n_items, n_ks = model.sess, model.sess.device, model.n_items, len(ks)
    expo, stats = sess.exposure_stats(bucket)
    m = torch.minimum(count.clamp(min=0).to(torch.int64)[:, None], torch.tensor(ks, dtype=torch.int64, device=dev)[None, :])
    pairs = m * (m - 1)
    ratio = torch.where(pairs > 0, linked.to(torch.float64) / pairs.clamp(min=1).to(torch.float64), torch.zeros((), dtype=torch.float64, device=dev))
    ils_sum, ils_rows = sess.tree_sum(ratio.contiguous()), (pairs > 0).sum(0)
    nov_sum = None
    if popularity is not None:
        info, seen = (torch.from_numpy(a).to(dev) for a in self_information(popularity, n_items))
        shown = (expo > 0) & seen[None, :]
        terms = torch.where(shown, expo.to(torch.float64) * info[None, :], torch.zeros((), dtype=torch.float64, device=dev))
        nov_sum = sess.tree_sum(terms.t().contiguous())
    sess.synchronize()
    st = [[int(v) for v in row] for row in stats.cpu().tolist()]
    covered, total, sq, big_r = ([row[f] % (1 << 64) for row in st] for f in range(4))
    out = {"ks": list(ks), "covered": covered, "total": total,
           "coverage": [c / n_items if n_items else 0.0 for c in covered],
           "gini": [2 * r / (n_items * t) - (n_items + 1) / n_items if t else 0.0 for r, t in zip(big_r, total)],
           "herfindahl": [q / t ** 2 if t else 0.0 for q, t in zip(sq, total)],
           "ils": [float(v) / float(r) if r else 0.0 for v, r in zip(ils_sum.cpu().tolist(), ils_rows.cpu().tolist())]}
    if nov_sum is not None:
        out["novelty"] = [float(v) / float(t) if t else 0.0 for v, t in zip(nov_sum.cpu().tolist(), total)]
    out.update({"per_user": {"linked": linked}, "exposure": expo, "bucket": bucket})
    return out


def list_metrics(model: DeviceModel, count: torch.Tensor, idx: torch.Tensor, ks: Sequence[int], popularity=None, chunk: int = 65536, bucket=None) -> dict:
    """The list metrics of a recommendation table (decision D35): count int32 [n], idx int32 [n, num] on the model's device -- any table, in particular
    the one user_recommendations(quota=...) returns.  ks: strictly ascending cut-offs inside 1..num, at most EVAL_MAX_KS.  Per cut-off, over the first k
    positions of every row: "coverage" (items shown at all / n_items), "gini" and "herfindahl" of the exposure (0 = every item shown equally often),
    "ils" (the mean over the rows of two or more entries of linked pairs / all ordered pairs, a pair (a, b) linked when the primary indicator row of a
    names b), "novelty" (only with popularity: the exposure-weighted mean of -log2(pop / sum of pop), see self_information); "covered" and "total" are
    the integers behind them, "per_user" {"linked" int32 [n, n_ks]}, "exposure" int64 [n_ks, n_items] and "bucket" the device tensors.  The table is
    walked `chunk` rows per call; nothing depends on chunk, and every number is reproducible bit for bit.  bucket: the "bucket" of an earlier report --
    the exposure then accumulates over both tables ("ils" and "per_user" describe this table alone).  Synchronises once, at the end."""
    ks = [int(k) for k in ks]
    if idx.dim() != 2 or idx.shape[0] != count.numel():
        raise ValueError("list_metrics: count [n] and idx [n, num] expected")
    if not 1 <= len(ks) <= _lib.EVAL_MAX_KS or ks[0] < 1 or ks[-1] > idx.shape[1] or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"ks: between 1 and {_lib.EVAL_MAX_KS} strictly ascending cut-offs inside 1..{idx.shape[1]}, got {ks}")
    if chunk < 1:
        raise ValueError("list_metrics needs chunk >= 1")
    n = int(count.numel())
    linked = torch.zeros((n, len(ks)), dtype=torch.int32, device=model.sess.device)
    if bucket is None:
        bucket = torch.zeros((len(ks), model.n_items), dtype=torch.uint32, device=model.sess.device)
    for lo in range(0, max(n, 1), chunk):
        bucket = _list_chunk(model, count[lo:lo + chunk], idx[lo:lo + chunk], ks, bucket, linked[lo:lo + chunk])
    return _list_report(model, ks, bucket, count, linked, popularity)


def evaluate(algo, model: DeviceModel, train, test, ks: Sequence[int] = (1, 5, 10, 20), num: Optional[int] = None, event_names=None,
             truth_event: Optional[str] = None, chunk: int = 65536, user_bias: Optional[float] = None, item_mask=None, now_ms: Optional[int] = None,
             term_weights=None, accumulator=None, list_metrics: bool = False, popularity=None):
    """Scores the model's recommendations for every user id of `train` (what user_recommendations answers over it, under `event_names` /
    `user_bias`) against the user's `truth_event` items in `test`.  train, test: DeviceHistory objects over ONE user id space.  truth_event:
    default the model's primary event; its stream in `test` carries the primary's item ids (no column map).  ks: strictly ascending cut-offs, at
    most EVAL_MAX_KS; num: the table's width, default max(ks).
    Returns {"ks", "evaluated", "not_evaluated" (users without a truth item: not part of any mean), "precision" (sum of hits / (evaluated k)),
    "hit_rate" (users with a hit / evaluated), "map", "ndcg" (the D19 tree sums / evaluated): a list per k, 0.0 when nobody was evaluated;
    "per_user": {"hits" int32, "ap", "ndcg" float64: device tensors [n_users, n_ks]}}.  event_names as a list of lists: one report per event mix,
    in a list -- the reference's predictiveness test of an indicator mix.  One synchronisation per chunk (the history calls' bound totals) and
    one at the end.  term_weights: passed to user_recommendations (decision D20) -- what the weights buy on a data set is measured by evaluating twice.
    accumulator: passed to user_recommendations (decision D31); the metrics do not depend on it.
    list_metrics: the report also holds the keys of list_metrics() over the same tables (decision D35; "per_user" gains "linked"), with "novelty" under
    `popularity`; the default leaves the report as it was."""
    if not isinstance(train, DeviceHistory) or not isinstance(test, DeviceHistory):
        raise ValueError("evaluate needs two history.DeviceHistory objects, the training and the held-out events")
    if train.n_users != test.n_users or train.user_dict is not test.user_dict or not (train.user_ids is test.user_ids or train.user_ids == test.user_ids):
        raise ValueError("train and test must share one user id space")      # (keyed histories: ONE dictionary object; append_keys({}) levels n_users)
    if event_names is not None and len(event_names) and all(isinstance(e, (list, tuple)) for e in event_names):
        return [evaluate(algo, model, train, test, ks, num, list(mix), truth_event, chunk, user_bias, item_mask, now_ms, term_weights, accumulator, list_metrics,
                         popularity) for mix in event_names]
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= _lib.EVAL_MAX_KS or ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"ks: between 1 and {_lib.EVAL_MAX_KS} strictly ascending cut-offs >= 1, got {ks}")
    num = int(num) if num is not None else ks[-1]
    if num < ks[-1] or num > _lib.REC_MAX_NUM:
        raise ValueError(f"num must lie in max(ks)..{_lib.REC_MAX_NUM}, got {num}")
    if chunk < 1:
        raise ValueError("evaluate needs chunk >= 1")
    truth_event = truth_event if truth_event is not None else list(algo.modelEventNames)[0]
    st = test.types.get(truth_event)
    if st is None:
        raise ValueError(f"the test history holds no stream of the truth event {truth_event!r}")
    if st.col_map is not None:
        raise ValueError(f"the test stream of {truth_event!r} must carry the primary event's item ids (it has a column map)")
    sess, dev = model.sess, model.sess.device
    n, n_ks = train.n_users, len(ks)
    discount = torch.from_numpy(log2_discount(num)).to(dev)
    hits = torch.zeros((n, n_ks), dtype=torch.int32, device=dev)
    ap = torch.zeros((n, n_ks), dtype=torch.float64, device=dev)
    ndcg = torch.zeros((n, n_ks), dtype=torch.float64, device=dev)
    sums_i = torch.zeros(2 + 2 * n_ks, dtype=torch.int64, device=dev)
    truth_spec = [(st.n_cols, TRUTH_CAP, False, st.idx_row_ptr, st.idx_pos, st.items, st.times, None)]
    if list_metrics:
        counts, linked, bucket = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros((n, n_ks), dtype=torch.int32, device=dev), None
    for lo in range(0, n, chunk):
        q = torch.arange(lo, min(lo + chunk, n), dtype=torch.int32, device=dev)
        count, idx, _ = user_recommendations(algo, model, train, q, num, event_names, user_bias, chunk, item_mask, now_ms, term_weights, accumulator=accumulator)
        (truth,), _, _ = sess.history_rows(q, test.n_users, truth_spec, model.n_items)
        hi = lo + int(q.numel())
        _, _, _, s_i, _ = sess.rank_metrics(count, idx, truth[0], truth[1], ks, discount, sums=True, out=(hits[lo:hi], ap[lo:hi], ndcg[lo:hi]))
        sums_i += s_i
        if list_metrics:
            counts[lo:hi] = count
            bucket = _list_chunk(model, count, idx, ks, bucket, linked[lo:hi])
    tree_ap, tree_ndcg = sess.tree_sum(ap), sess.tree_sum(ndcg)
    sess.synchronize()
    report = _report(ks, sums_i.cpu().tolist(), tree_ap.cpu().tolist(), tree_ndcg.cpu().tolist(), {"hits": hits, "ap": ap, "ndcg": ndcg})
    if list_metrics:
        if bucket is None:
            bucket = torch.zeros((n_ks, model.n_items), dtype=torch.uint32, device=dev)
        extra = _list_report(model, ks, bucket, counts, linked, popularity)
        report["per_user"].update(extra.pop("per_user"))
        report.update(extra)
    return report


def split_streams(streams: Dict[str, Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]], at_ms: int):
    """(before, from): two dicts of the DeviceHistory.from_streams form, the events with time < at_ms and those with time >= at_ms of every
    stream, in stream order.  Tensor masks only; a stream without times cannot be split: ValueError."""
    before, later = {}, {}
    for ev, (users, items, times) in streams.items():
        if times is None:
            raise ValueError(f"stream {ev!r} has no times: it cannot be split at a time")
        early = times < int(at_ms)
        before[ev] = (users[early], items[early], times[early])
        later[ev] = (users[~early], items[~early], times[~early])
    return before, later
