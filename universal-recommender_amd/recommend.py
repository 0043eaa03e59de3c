"""The query half of the Universal Recommender in batch form, on the GPU that holds the model (reference
URAlgorithm.predict / buildQuery* / get*, src/main/scala/URAlgorithm.scala:484-953; the `pio batchpredict` use case).

The reference turns a query into an Elasticsearch bool query: one `terms` should-clause per (event, id list, boost), must_not ids, a
popularity sort behind `_score`.  Here the same clauses are rows of sparse 0/1 matrices and urcco_dev_recommend (include/urcco.h) forms
    score(q, i) = sum over clauses c, in call order, of boost_c * |T_c(q) ^ I_c(i)|
against the indicator matrices the build left in HBM: an item has a positive score exactly when Elasticsearch gives it one; magnitudes and
the order among positives are this library's (decision D15 of DESIGN.md -- BM25's `_score` cannot be reproduced).  PyTorch is plumbing here
(device memory, the argsort of the backfill ranks); the product and the top-k are hand-written HIP.

Not served (NotImplementedError names the key): query `fields` (property boost / filter / exclude), `dateRange`, negative user / item bias
(history used as a filter).  Items outside the primary event's item dictionary are never returned."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .device import DevCsr, DevIndicators, DeviceSession
from .indexed_dataset import BiDictionary, IndexedDataset


@dataclass
class _Correlator:
    name: str
    n_cols: int
    column_ids: Optional[BiDictionary]
    col_ptr: torch.Tensor          # CSC of the indicator matrix, device
    row_idx: torch.Tensor
    row_ptr: torch.Tensor          # its CSR (device): the query item's own indicator lists are read from it
    col_idx: torch.Tensor
    host: Optional[Tuple[np.ndarray, np.ndarray]] = None   # (row_ptr, col_idx) on the host, fetched once


class DeviceModel:
    """The indicator matrices of a built model in HBM, in the form urcco_dev_recommend reads (CSC), with their dictionaries."""

    def __init__(self, sess: DeviceSession, item_ids: Optional[BiDictionary], n_items: int, correlators: List[_Correlator], fill_order: Optional[torch.Tensor]):
        self.sess, self.item_ids, self.n_items, self.correlators, self.fill_order = sess, item_ids, n_items, correlators, fill_order
        self.by_name = {c.name: c for c in correlators}

    @staticmethod
    def from_indicators(sess: DeviceSession, correlators: Sequence[Tuple[str, object]], ranks: Optional[Dict[object, float]] = None,
                        item_ids: Optional[BiDictionary] = None, column_ids: Optional[Dict[str, BiDictionary]] = None) -> "DeviceModel":
        """correlators: (event name, IndexedDataset | DevIndicators) per event type, the primary first -- URModel.coocurrenceMatrices or the device
        build's own output (then the dictionaries come through item_ids / column_ids; without them ids are the dense integers).
        ranks: {item: rank} (popRank of calcAll's properties) -> the backfill order: rank desc, items without a rank last, then item index."""
        if not correlators:
            raise ValueError("a model needs at least the primary event's indicator matrix")
        out: List[_Correlator] = []
        n_items = None
        for name, ind in correlators:
            if isinstance(ind, IndexedDataset):
                rows, n_cols = ind.nrow, ind.ncol
                nnz = ind.nnz
                rp = torch.from_numpy(ind.row_ptr).to(sess.device)
                ci = torch.from_numpy(ind.col_idx[:nnz] if nnz else np.zeros(1, np.int32)).to(sess.device)
                cids, host = ind.columnIDs, (ind.row_ptr, ind.col_idx)
                if item_ids is None:
                    item_ids = ind.rowIDs
            elif isinstance(ind, DevIndicators):
                if ind.item_lo != 0:
                    raise ValueError("a DeviceModel needs whole indicator matrices (item_lo == 0)")
                rows, n_cols = ind.item_hi, ind.n_cols
                rp, ci = ind.row_ptr, ind.col_idx
                nnz = int(rp[-1].item()) if rows else 0     # entries past row_ptr[-1] are capacity, not part of the matrix
                cids, host = (column_ids or {}).get(name), None
            else:
                raise TypeError(f"indicator matrix of {name!r}: IndexedDataset or DevIndicators expected")
            if n_items is None:
                n_items = rows
            elif rows != n_items:
                raise ValueError("every indicator matrix has one row per item of the primary event")
            m = DevCsr(rows, n_cols, rp, ci, nnz)
            counts = sess.column_counts(ci, nnz, n_cols, sess.empty(max(n_cols, 1), torch.int32))
            cp, ri = sess.transpose(m, counts)
            out.append(_Correlator(name, n_cols, cids, cp, ri, rp, ci, host))
        fill = None
        if ranks:
            r = torch.full((n_items,), float("-inf"), dtype=torch.float64)
            for item, v in ranks.items():
                i = item_ids.get(item) if item_ids is not None else int(item)
                if i is not None and 0 <= i < n_items:
                    r[i] = float(v)
            fill = torch.sort(-r.to(sess.device), stable=True).indices.to(torch.int32)
        return DeviceModel(sess, item_ids, n_items, out, fill)

    # ---- dictionaries ----
    def item_index(self, item) -> Optional[int]:
        if self.item_ids is not None:
            return self.item_ids.get(item)
        try:
            i = int(item)
        except (TypeError, ValueError):
            return None
        return i if 0 <= i < self.n_items else None

    def item_name(self, i: int):
        return self.item_ids.inverse(i) if self.item_ids is not None else i

    def column_index(self, c: _Correlator, key) -> Optional[int]:
        if c.column_ids is not None:
            return c.column_ids.get(key)
        try:
            i = int(key)
        except (TypeError, ValueError):
            return None
        return i if 0 <= i < c.n_cols else None

    def indicator_row(self, c: _Correlator, i: int) -> np.ndarray:
        """Column indices of item i's indicator list for this event, strongest first (one read of the matrix per model)."""
        if c.host is None:
            rp = c.row_ptr.cpu().numpy()
            c.host = (rp, c.col_idx[: max(int(rp[-1]), 1)].cpu().numpy())
        rp, ci = c.host
        return ci[rp[i]:rp[i + 1]]


def _csr(rows: List[np.ndarray], device) -> Tuple[torch.Tensor, torch.Tensor]:
    rp = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([r.size for r in rows], out=rp[1:])
    ci = np.concatenate(rows).astype(np.int32) if rp[-1] else np.zeros(1, np.int32)
    return torch.from_numpy(rp).to(device), torch.from_numpy(ci).to(device)


def _boost(bias: float) -> float:
    """URAlgorithm.scala:777-779, :824-825: a bias > 0 and != 1 is the boost, everything else leaves the clause unboosted."""
    return float(bias) if bias > 0 and bias != 1 else 1.0


def batch_predict(algo, model: DeviceModel, queries: Sequence[dict], history: Dict[str, Dict[str, List[str]]], item_mask=None) -> List[dict]:
    """URAlgorithm.predict for a list of query dicts: [{"itemScores": [{"item", "score"}, ...]}, ...] in the order of `queries`.
    history: user -> {event name: [item ids, oldest first]} (the event store's view of the user); item_mask: None, an array of n_items
    flags or {item: bool} (the available / expire date filter evaluated for "now"; items not named are eligible)."""
    ap = algo.ap
    model_events = list(algo.modelEventNames)
    primary = model_events[0]
    for ev in model_events:
        if ev not in model.by_name:
            raise ValueError(f"the model holds no indicator matrix for event {ev!r}")
    max_items = {i.name: (i.maxItemsPerUser if i.maxItemsPerUser is not None else 500) for i in ap.indicators} if ap.indicators else {e: 100 for e in model_events}
    if ap.indicators:                                                                          # :203-211
        max_query_events = sum(i.maxItemsPerUser if i.maxItemsPerUser is not None else 100 for i in ap.indicators) * 10
    else:
        max_query_events = ap.maxQueryEvents if ap.maxQueryEvents is not None else 100
    limit = ap.num if ap.num is not None else 20
    blacklist_events = ap.blacklistEvents if ap.blacklistEvents is not None else [primary]      # :236
    flags = _lib.REC_NO_BACKFILL if algo.recsModel == "collabFiltering" else 0

    mask_t = None
    if item_mask is not None:
        if isinstance(item_mask, dict):
            m = np.ones(model.n_items, np.uint8)
            for item, ok in item_mask.items():
                i = model.item_index(item)
                if i is not None:
                    m[i] = 1 if ok else 0
            mask_t = torch.from_numpy(m).to(model.sess.device)
        else:
            mask_t = torch.as_tensor(np.asarray(item_mask) != 0 if not torch.is_tensor(item_mask) else item_mask != 0).to(torch.uint8).to(model.sess.device)
            if mask_t.numel() != model.n_items:
                raise ValueError("item_mask needs one flag per item of the primary event")

    # ---- per query: clause terms, exclusions, and the key of the call it can share ----
    groups: Dict[tuple, List[int]] = {}
    plans = []
    for n, q in enumerate(queries):
        for key in ("fields", "dateRange"):
            if q.get(key):
                raise NotImplementedError(f"query key {key!r} is not served by batch_predict")
        user_bias = q.get("userBias", ap.userBias if ap.userBias is not None else 1.0)
        item_bias = q.get("itemBias", ap.itemBias if ap.itemBias is not None else 1.0)
        if user_bias < 0:
            raise NotImplementedError("negative userBias (user history as a filter) is not served by batch_predict")
        if item_bias < 0:
            raise NotImplementedError("negative itemBias (similar items as a filter) is not served by batch_predict")
        num = int(q.get("num", limit))
        start = int(q.get("from", 0))
        if num < 1 or start < 0:
            raise ValueError(f"query {n}: num must be >= 1 and from >= 0")
        if start + num > _lib.REC_MAX_NUM:
            raise ValueError(f"query {n}: from + num = {start + num} exceeds {_lib.REC_MAX_NUM}")
        q_events = list(q.get("eventNames") or model_events)
        user, item, item_set = q.get("user"), q.get("item"), list(q.get("itemSet") or [])
        terms: Dict[tuple, np.ndarray] = {}
        excl: List[int] = []
        events = history.get(user, {}) if user is not None else {}
        for ev in q_events:                                                                     # getBiasedRecentUserActions :795-839
            c = model.by_name.get(ev)
            if c is None:
                continue
            recent = list(reversed(events.get(ev, [])))[: max_items.get(ev, 100)]               # most recent first, capped, then distinct
            ids = [model.column_index(c, i) for i in dict.fromkeys(recent)]
            terms[("user", ev)] = np.unique(np.array([i for i in ids if i is not None], np.int64))
        for ev in q_events:                                                                     # getExcludedItems :741-767
            if ev in blacklist_events:
                excl += [model.item_index(i) for i in events.get(ev, [])]
        excl += [model.item_index(i) for i in (q.get("blacklistItems") or [])]
        if item is not None:
            i = model.item_index(item)
            if i is not None:                                                                   # getBiasedSimilarItems :770-792
                for ev in model_events:
                    c = model.by_name[ev]
                    ids = model.indicator_row(c, i)
                    if ids.size > max_query_events:
                        ids = ids[: max_query_events - 1]
                    terms[("item", ev)] = np.unique(ids.astype(np.int64))
            if not q.get("returnSelf", ap.returnSelf if ap.returnSelf is not None else False):
                excl.append(i)
        if item_set:                                                                            # :645
            c = model.by_name[primary]
            ids = [model.column_index(c, i) for i in item_set]
            terms[("set", primary)] = np.unique(np.array([i for i in ids if i is not None], np.int64))
            excl += [model.item_index(i) for i in item_set]
        set_bias = q.get("itemSetBias", 1.0)
        if set_bias is None or set_bias < 0:
            set_bias = 1.0
        key = (_boost(user_bias), _boost(item_bias), _boost(set_bias), start + num)
        groups.setdefault(key, []).append(n)
        plans.append((terms, np.unique(np.array([i for i in excl if i is not None], np.int64)), start, num))

    # ---- one call per group ----
    results: List[Optional[dict]] = [None] * len(queries)
    dev = model.sess.device
    empty = np.zeros(0, np.int64)
    for (ub, ib, sb, fetch), members in groups.items():
        slots = []
        for kind, boost in (("user", ub), ("item", ib), ("set", sb)):
            for ev in ([primary] if kind == "set" else model_events if kind == "item" else list(model.by_name)):
                if any(plans[n][0].get((kind, ev), empty).size for n in members):
                    slots.append((kind, ev, boost))
        if len(slots) > _lib.REC_MAX_CLAUSES:
            raise ValueError(f"a batch needs {len(slots)} clauses, more than the {_lib.REC_MAX_CLAUSES} one call serves")
        clauses = []
        for kind, ev, boost in slots:
            c = model.by_name[ev]
            qrp, qci = _csr([plans[n][0].get((kind, ev), empty) for n in members], dev)
            clauses.append((c.n_cols, boost, c.col_ptr, c.row_idx, qrp, qci))
        excl = _csr([plans[n][1] for n in members], dev)
        count, idx, score, _ = model.sess.recommend(len(members), model.n_items, clauses, fetch, excl, mask_t, model.fill_order, flags, stats=False)
        model.sess.synchronize()
        count, idx, score = count.cpu().numpy(), idx.cpu().numpy(), score.cpu().numpy()
        for r, n in enumerate(members):
            start, num = plans[n][2], plans[n][3]
            results[n] = {"itemScores": [{"item": model.item_name(int(idx[r, j])), "score": float(score[r, j])} for j in range(start, min(int(count[r]), start + num))]}
    return results
