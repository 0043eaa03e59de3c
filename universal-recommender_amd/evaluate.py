"""Hold-out evaluation of a built model on the GPU that holds it: MAP@k, NDCG@k, precision and hit rate over the users of a test history
(decision D19 of DESIGN.md; include/urcco.h urcco_dev_rank_metrics).

The reference leaves this to its MAP@k tool, for which its query key `eventNames` exists ("for indicator predictiveness testing",
URAlgorithm.scala:401 `queryEventNames`): train on the events before a split, ask for every user's recommendations under an event mix, and score
them against what the user did afterwards.  Here the users' recommendations come from recommend.user_recommendations over the training
history, the held-out sets are the test history's term rows of the truth event (decision D17, cap 2^31 - 1: every event), and
urcco_dev_rank_metrics scores `chunk` users per call.  The per-user values of all chunks land in one [n_users, n_ks] tensor per metric and
urcco_dev_tree_sum adds each column once, in the fixed pairwise order of the decision: the report does not depend on `chunk`, and every number
in it is reproducible bit for bit."""
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


def evaluate(algo, model: DeviceModel, train, test, ks: Sequence[int] = (1, 5, 10, 20), num: Optional[int] = None, event_names=None,
             truth_event: Optional[str] = None, chunk: int = 65536, user_bias: Optional[float] = None, item_mask=None, now_ms: Optional[int] = None,
             term_weights=None):
    """Scores the model's recommendations for every user id of `train` (what user_recommendations answers over it, under `event_names` /
    `user_bias`) against the user's `truth_event` items in `test`.  train, test: DeviceHistory objects over ONE user id space.  truth_event:
    default the model's primary event; its stream in `test` carries the primary's item ids (no column map).  ks: strictly ascending cut-offs, at
    most EVAL_MAX_KS; num: the table's width, default max(ks).
    Returns {"ks", "evaluated", "not_evaluated" (users without a truth item: not part of any mean), "precision" (sum of hits / (evaluated k)),
    "hit_rate" (users with a hit / evaluated), "map", "ndcg" (the D19 tree sums / evaluated): a list per k, 0.0 when nobody was evaluated;
    "per_user": {"hits" int32, "ap", "ndcg" float64: device tensors [n_users, n_ks]}}.  event_names as a list of lists: one report per event mix,
    in a list -- the reference's predictiveness test of an indicator mix.  One synchronisation per chunk (the history calls' bound totals) and
    one at the end.  term_weights: passed to user_recommendations (decision D20) -- what the weights buy on a data set is measured by evaluating twice."""
    if not isinstance(train, DeviceHistory) or not isinstance(test, DeviceHistory):
        raise ValueError("evaluate needs two history.DeviceHistory objects, the training and the held-out events")
    if train.n_users != test.n_users or train.user_dict is not test.user_dict or not (train.user_ids is test.user_ids or train.user_ids == test.user_ids):
        raise ValueError("train and test must share one user id space")      # (keyed histories: ONE dictionary object; append_keys({}) levels n_users)
    if event_names is not None and len(event_names) and all(isinstance(e, (list, tuple)) for e in event_names):
        return [evaluate(algo, model, train, test, ks, num, list(mix), truth_event, chunk, user_bias, item_mask, now_ms, term_weights) for mix in event_names]
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
    for lo in range(0, n, chunk):
        q = torch.arange(lo, min(lo + chunk, n), dtype=torch.int32, device=dev)
        count, idx, _ = user_recommendations(algo, model, train, q, num, event_names, user_bias, chunk, item_mask, now_ms, term_weights)
        (truth,), _, _ = sess.history_rows(q, test.n_users, truth_spec, model.n_items)
        hi = lo + int(q.numel())
        _, _, _, s_i, _ = sess.rank_metrics(count, idx, truth[0], truth[1], ks, discount, sums=True, out=(hits[lo:hi], ap[lo:hi], ndcg[lo:hi]))
        sums_i += s_i
    tree_ap, tree_ndcg = sess.tree_sum(ap), sess.tree_sum(ndcg)
    sess.synchronize()
    return _report(ks, sums_i.cpu().tolist(), tree_ap.cpu().tolist(), tree_ndcg.cpu().tolist(), {"hits": hits, "ap": ap, "ndcg": ndcg})


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
