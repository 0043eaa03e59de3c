"""The query half of the Universal Recommender in batch form, on the GPU that holds the model (reference
URAlgorithm.predict / buildQuery* / get*, src/main/scala/URAlgorithm.scala:484-953; the `pio batchpredict` use case).

The reference turns a query into an Elasticsearch bool query: one `terms` should-clause per (event, id list, boost), must_not ids, a
popularity sort behind `_score`.  Here the same clauses are rows of sparse 0/1 matrices and urcco_dev_recommend (include/urcco.h) forms
    score(q, i) = sum over clauses c, in call order, of boost_c * |T_c(q) ^ I_c(i)|
against the indicator matrices the build left in HBM: an item has a positive score exactly when Elasticsearch gives it one; magnitudes and
the order among positives are this library's (decision D15 of DESIGN.md -- BM25's `_score` cannot be reproduced).  PyTorch is plumbing here
(device memory, the argsort of the backfill ranks); the product and the top-k are hand-written HIP.

Business rules (decision D16; buildQueryMust / buildQueryMustNot / getBoostedMetadata / getFilteringDateRange, :684-727, :841-953) are served
by a model built with item properties (`DeviceModel.from_indicators(..., properties=..., date_names=...)`): they become eligibility rules that
urcco_dev_recommend_rules evaluates on the device per (query, item), inside the top-`num` cut and the backfill walk:
    fields, bias > 0     one more should-clause over the property's item x value matrix, boost = bias, after the similar-item clauses (:653)
    fields, bias < 0     ANY rule: the item holds one of the values          fields, bias == 0    NONE rule: the item holds none of them
    dateRange            RANGE rule on the named date: after < date < before, a missing side open; an item without the date fails
    no dateRange, availableDateName and expireDateName configured and held by the model: available <= now and expire > now, now = the query's
                         currentDate, else `now_ms`, else the wall clock (the reference's `else if`: a dateRange replaces this rule, :877-948)
    userBias < 0         one ANY rule per query event: the item's indicator list for the event holds one of the user's recent items -- not a
                         should-clause; an event without history matches nothing, as an empty `terms` query does (:688-693)
    itemBias < 0         the same with the query item's own indicator lists (:695-699)
An unknown property name or value has no column: an ANY on it matches nothing, a NONE or a boost on it does nothing.  A model built WITHOUT
properties raises NotImplementedError (naming the key) for all of these, as before.

Term weights (decision D20): every entry point takes `term_weights`.  None scores every matching term 1 (D15, the calls above).  "idf" weighs a term by
its rarity -- DeviceModel.term_weights: Lucene's BM25 idf of the term among the items whose field is not empty, as urcco_dev_idf_weights rounds it to
units of 2^-15 -- and a dict {event or property name: uint32 device tensor, one weight per column} gives the caller's own.  Every should-clause then
carries the array of its matrix (user history, similar items, item set: the event's; a boosted `fields` clause: the property's) and the call is
urcco_dev_recommend_weighted; ANY / NONE rules are filters and carry no weight.  Ids and score bits stay reproducible.  It is NOT Elasticsearch's BM25:
the length norm and the per-shard statistics are left out.  Not served: engine.json-level `fields`.  Items outside the
primary event's item dictionary are never returned."""
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


@dataclass
class _Property:
    """A list-of-strings item property as an item x value 0/1 matrix on the device: CSR for the rules, CSC for boost clauses."""
    name: str
    n_cols: int
    values: Dict[str, int]
    row_ptr: torch.Tensor
    col_idx: torch.Tensor
    col_ptr: torch.Tensor
    row_idx: torch.Tensor


NO_VALUE = -(1 << 63)      # INT64_MIN: the item has no value for a RANGE rule
OPEN_HI = (1 << 63) - 1


class DeviceModel:
    """The indicator matrices of a built model in HBM, in the form urcco_dev_recommend reads (CSC), with their dictionaries."""

    def __init__(self, sess: DeviceSession, item_ids: Optional[BiDictionary], n_items: int, correlators: List[_Correlator], fill_order: Optional[torch.Tensor],
                 properties: Optional[Dict[str, _Property]] = None, dates: Optional[Dict[str, torch.Tensor]] = None):
        self.sess, self.item_ids, self.n_items, self.correlators, self.fill_order = sess, item_ids, n_items, correlators, fill_order
        self.by_name = {c.name: c for c in correlators}
        self.properties = properties    # None: built without item properties -- batch_predict serves no business rules
        self.dates = dates or {}        # date property -> int64 [n_items] epoch milliseconds, NO_VALUE where the item has none
        self._term_weights: Dict[str, Dict[str, torch.Tensor]] = {}   # term_weights(kind), built on first use
        self.rank_fields: Dict[str, torch.Tensor] = {}   # set_ranks: ranking field name -> int64 [n_items], _lib.RANK_NONE = no rank
        self._key_dicts: Dict[str, object] = {}          # key_dictionary(ev), built on first use

    def set_ranks(self, fields: Dict[str, torch.Tensor]) -> "DeviceModel":
        """The backfill order from rank fields on the device (decision D24 of DESIGN.md): fields = {ranking field name: int64 device tensor [n_items],
        _lib.RANK_NONE where the item has no rank}, in the order of the reference's rankingFieldNames -- what history.DeviceHistory.ranks returns.  The
        tensors are kept as rank_fields and fill_order becomes the items sorted by every field in turn, larger rank first, an item without a rank last,
        then item index (`sort: [_score desc, <each ranking field> desc]`, URAlgorithm.scala:730-738) -- DeviceSession.fill_order.  Nothing else of the
        model changes and nothing is rebuilt: a serving model takes fresh trending / hot ranks between two trainings.  {} clears both.  Returns self."""
        fields = dict(fields)
        for name, r in fields.items():
            if r.dtype != torch.int64 or int(r.numel()) != self.n_items:
                raise ValueError(f"rank field {name!r}: an int64 tensor with one entry per item of the primary expected")
        self.rank_fields = fields
        self.fill_order = self.sess.fill_order(list(fields.values())) if fields else None
        return self

    def set_properties(self, props) -> "DeviceModel":
        """The item properties of a serving model from a properties.DeviceProperties (decision D25 of DESIGN.md): `properties` and `dates` become what
        props.materialise() cuts from the property events aggregated on the device -- an item that sold out, changed category or got a new expire date
        reaches the rules without a rebuild.  The cached term weights are dropped: the idf arrays of the property matrices depend on them.  Nothing else
        of the model changes; the "deleted" mask is props.item_mask(), for batch_predict(item_mask=...).  Returns self."""
        if int(props.n_items) != self.n_items:
            raise ValueError("the properties hold another number of items than the model")
        self.properties, self.dates = props.materialise()
        self._term_weights = {}
        return self

    @staticmethod
    def from_indicators(sess: DeviceSession, correlators: Sequence[Tuple[str, object]], ranks: Optional[Dict[object, float]] = None,
                        item_ids: Optional[BiDictionary] = None, column_ids: Optional[Dict[str, BiDictionary]] = None,
                        properties: Optional[Dict[object, Dict[str, object]]] = None, date_names: Sequence[str] = ()) -> "DeviceModel":
        """correlators: (event name, IndexedDataset | DevIndicators) per event type, the primary first -- URModel.coocurrenceMatrices or the device
        build's own output (then the dictionaries come through item_ids / column_ids; without them ids are the dense integers).
        ranks: {item: rank} (popRank of calcAll's properties) -> the backfill order: rank desc, items without a rank last, then item index.
        properties: item -> {name: value} (URModel.propertiesMaps[0]) -> the business rules of batch_predict: every list-of-strings property becomes
        an item x value matrix on the device, every name in date_names an int64 array of epoch milliseconds (URModel.extractJvalue parses the
        strings).  Items outside the primary's dictionary and other properties are ignored.  None: no rules are served ({} serves the negative
        biases alone)."""
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
        model = DeviceModel(sess, item_ids, n_items, out, fill)
        if properties is not None:
            model.properties, model.dates = _device_properties(sess, properties, date_names, n_items, model.item_index)
        return model

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

    def key_dictionary(self, ev: str):
        """The device dictionary 64-bit key -> column id of an event type (decision D26 of DESIGN.md): preparator.hash_keys of the strings of its column_ids in
        id order -- of item_ids for an event name outside the model -- built once, on first use.  First-appearance ids over distinct strings in id order
        ARE those ids, so a lookup of an item's key answers its column id, and -1 for a key outside the catalogue.  ValueError: the model carries no
        strings for that id space; ingest.HashCollision: two of them share a key."""
        from . import ingest
        from .preparator import hash_keys
        d = self._key_dicts.get(ev)
        if d is None:
            c = self.by_name.get(ev)
            names = c.column_ids if c is not None else self.item_ids
            if names is None:
                raise ValueError(f"event {ev!r}: the model was built over dense integer ids, it has no strings to key")
            keys = torch.from_numpy(hash_keys(names.keys, library=self.sess.lib)).to(self.sess.device)
            d = ingest.dictionary_build(self.sess, keys)
            if d.n_ids != len(names):
                d.close()
                raise ingest.HashCollision(f"event {ev!r}: two item ids share a 64-bit key")
            self._key_dicts[ev] = d
        return d

    def term_weights(self, kind: str = "idf") -> Dict[str, torch.Tensor]:
        """{event name or list-of-strings property name: uint32 device tensor [n_cols]}: the term weights of decision D20 for every matrix a should-clause
        can be built on, in units of 2^-15.  kind "idf": urcco_dev_idf_weights over the matrix's CSC with n_docs = the items whose row of the matrix is not
        empty (Elasticsearch's doc count of the field; at least 1), read from the CSR row_ptr the model holds.  Built on first use and cached; where a
        property shares its name with an event type, the event's array is the one under the name."""
        if kind != "idf":
            raise ValueError(f"term weights of kind {kind!r} are not known ('idf' is)")
        if kind not in self._term_weights:
            out: Dict[str, torch.Tensor] = {}
            for m in list((self.properties or {}).values()) + list(self.correlators):
                rp = m.row_ptr[: self.n_items + 1]
                n_docs = int((rp[1:] > rp[:-1]).sum().item()) if self.n_items else 0
                out[m.name] = self.sess.idf_weights(m.col_ptr, m.n_cols, max(n_docs, 1))
            self._term_weights[kind] = out
        return self._term_weights[kind]

    def indicator_row(self, c: _Correlator, i: int) -> np.ndarray:
        """Column indices of item i's indicator list for this event, strongest first (one read of the matrix per model)."""
        if c.host is None:
            rp = c.row_ptr.cpu().numpy()
            c.host = (rp, c.col_idx[: max(int(rp[-1]), 1)].cpu().numpy())
        rp, ci = c.host
        return ci[rp[i]:rp[i + 1]]


def _device_properties(sess: DeviceSession, properties, date_names: Sequence[str], n_items: int, index_of):
    from .ur_model import extractJvalue
    lists: Dict[str, Tuple[Dict[str, int], List[Tuple[int, int]]]] = {}
    dates = {name: np.full(n_items, NO_VALUE, np.int64) for name in date_names}
    for item, fields in properties.items():
        i = index_of(item)
        if i is None:
            continue
        for name, value in fields.items():
            if name in dates:
                if isinstance(value, str):
                    dates[name][i] = int(round(extractJvalue(date_names, name, value).timestamp() * 1000))
            elif isinstance(value, (list, tuple)) and all(isinstance(v, str) for v in value):
                values, pairs = lists.setdefault(name, ({}, []))
                pairs += [(i, values.setdefault(v, len(values))) for v in value]
    props = {}
    for name, (values, pairs) in lists.items():
        if not values:
            continue
        key = np.unique(np.array([i * len(values) + v for i, v in pairs], np.int64))
        rp = np.zeros(n_items + 1, np.int64)
        np.cumsum(np.bincount(key // len(values), minlength=n_items), out=rp[1:])
        row_ptr = torch.from_numpy(rp).to(sess.device)
        col_idx = torch.from_numpy((key % len(values)).astype(np.int32)).to(sess.device)
        counts = sess.column_counts(col_idx, key.size, len(values), sess.empty(len(values), torch.int32))
        cp, ri = sess.transpose(DevCsr(n_items, len(values), row_ptr, col_idx, key.size), counts)
        props[name] = _Property(name, len(values), values, row_ptr, col_idx, cp, ri)
    return props, {name: torch.from_numpy(v).to(sess.device) for name, v in dates.items()}


def _csr(rows: List[np.ndarray], device) -> Tuple[torch.Tensor, torch.Tensor]:
    rp = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([r.size for r in rows], out=rp[1:])
    ci = np.concatenate(rows).astype(np.int32) if rp[-1] else np.zeros(1, np.int32)
    return torch.from_numpy(rp).to(device), torch.from_numpy(ci).to(device)


def _boost(bias: float) -> float:
    """URAlgorithm.scala:777-779, :824-825: a bias > 0 and != 1 is the boost, everything else leaves the clause unboosted."""
    return float(bias) if bias > 0 and bias != 1 else 1.0


def _date_ms(text: str, what: str) -> int:
    from .ur_algorithm import _iso_ms
    ms = _iso_ms(text)
    if ms is None:
        raise ValueError(f"{what}: {text!r} is not an ISO-8601 date")
    return ms


def _mask_tensor(model: DeviceModel, item_mask) -> Optional[torch.Tensor]:
    """None, an array of n_items flags or {item: bool} -> uint8 [n_items] on the model's device"""
    if item_mask is None:
        return None
    if isinstance(item_mask, dict):
        m = np.ones(model.n_items, np.uint8)
        for item, ok in item_mask.items():
            i = model.item_index(item)
            if i is not None:
                m[i] = 1 if ok else 0
        return torch.from_numpy(m).to(model.sess.device)
    mask_t = torch.as_tensor(np.asarray(item_mask) != 0 if not torch.is_tensor(item_mask) else item_mask != 0).to(torch.uint8).to(model.sess.device)
    if mask_t.numel() != model.n_items:
        raise ValueError("item_mask needs one flag per item of the primary event")
    return mask_t


def _term_weights(algo, model: DeviceModel, term_weights) -> Optional[Dict[str, torch.Tensor]]:
    """None (the algorithm's termWeights parameter decides; absent: unweighted), "none", "idf" or {name: uint32 device tensor} -> None = the unweighted
    calls, or the dict the clauses look their matrix's name up in (a name it does not hold: every term of that clause weighs 1.0)"""
    if term_weights is None:
        term_weights = getattr(algo.ap, "termWeights", None)
    if term_weights is None or (isinstance(term_weights, str) and term_weights == "none"):
        return None
    if isinstance(term_weights, str):
        return model.term_weights(term_weights)
    if not isinstance(term_weights, dict):
        raise ValueError("term_weights: None, 'none', 'idf' or a dict {event or property name: uint32 device tensor}")
    sizes = {m.name: m.n_cols for m in list((model.properties or {}).values()) + list(model.correlators)}
    for name, w in term_weights.items():
        if not torch.is_tensor(w) or w.dtype != torch.uint32 or w.dim() != 1 or w.device != model.sess.device or w.numel() != sizes.get(name, w.numel()):
            raise ValueError(f"term_weights[{name!r}]: a uint32 tensor on the model's device with one weight per column of the matrix")
    return term_weights


def _max_query_events(ap) -> int:
    if ap.indicators:                                                                          # :203-211
        return sum(i.maxItemsPerUser if i.maxItemsPerUser is not None else 100 for i in ap.indicators) * 10
    return ap.maxQueryEvents if ap.maxQueryEvents is not None else 100


def batch_predict(algo, model: DeviceModel, queries: Sequence[dict], history, item_mask=None, now_ms: Optional[int] = None, item_rows: str = "host",
                  term_weights=None) -> List[dict]:
    """URAlgorithm.predict for a list of query dicts: [{"itemScores": [{"item", "score"}, ...]}, ...] in the order of `queries`.
    history: user -> {event name: [item ids, oldest first]} (the event store's view of the user), or a history.DeviceHistory: the event streams
    resident on the device.  With a DeviceHistory the user-history term rows (the ("user", ev) clauses, or the ("hist", ev) ANY rules under
    userBias < 0) and the blacklist events' part of the exclusions come from one urcco_dev_history_bounds + _rows call per group (decision D17);
    blacklistItems, the query item and the item set go into that call as its extra exclusion rows.  Queries then share a call only when they name
    the same event types, and a group in which any member names a user carries the user clause of EVERY event type of the query, also where all
    its rows turn out empty (the dict form leaves such a clause out): an all-empty clause adds 0.0 * boost and leaves every score bit-identical,
    but the 16-clause limit of a call can be reached earlier than with the dict form.  item_mask: None, an array of n_items
    flags or {item: bool} (any further filter of the caller's; items not named are eligible -- it applies on top of the rules); now_ms: "now" of the
    available / expire rule for queries without `currentDate` (default: the wall clock).
    item_rows: "host" (default) plans the query item's own indicator lists one by one from a host copy of the matrices (DeviceModel.indicator_row; its
    first use copies every indicator matrix back from the device).  "device" cuts them on the device (decision D18): the ("item", ev) clause rows, or the
    ("sim", ev) ANY-rule rows under itemBias < 0, of a group come from one urcco_dev_item_bounds + _rows call per group over the group's dense item
    ids (-1 for a member without a known item), with max_terms = maxQueryEvents; no matrix comes back to the host.  A group in which any member names a
    known item then carries the item clause of EVERY event type of the model, also where all its rows turn out empty (the host route leaves such a
    clause out): an all-empty clause adds 0.0 * boost, so every score stays bit-identical to the host route, but the 16-clause limit of a call can be
    reached earlier.
    term_weights: None (the algorithm's termWeights parameter, absent: every matching term scores 1 -- the calls are then the unweighted ones), "none",
    "idf" (DeviceModel.term_weights) or {event or property name: uint32 device tensor}: decision D20, see the module's head."""
    tw = _term_weights(algo, model, term_weights)
    if item_rows not in ("host", "device"):
        raise ValueError(f"item_rows must be 'host' or 'device', got {item_rows!r}")
    dev_items = item_rows == "device"
    ap = algo.ap
    model_events = list(algo.modelEventNames)
    primary = model_events[0]
    for ev in model_events:
        if ev not in model.by_name:
            raise ValueError(f"the model holds no indicator matrix for event {ev!r}")
    max_items = {i.name: (i.maxItemsPerUser if i.maxItemsPerUser is not None else 500) for i in ap.indicators} if ap.indicators else {e: 100 for e in model_events}
    max_query_events = _max_query_events(ap)
    if dev_items and max_query_events < 1:
        raise ValueError("item_rows='device' needs maxQueryEvents >= 1")
    limit = ap.num if ap.num is not None else 20
    blacklist_events = ap.blacklistEvents if ap.blacklistEvents is not None else [primary]      # :236
    flags = _lib.REC_NO_BACKFILL if algo.recsModel == "collabFiltering" else 0

    mask_t = _mask_tensor(model, item_mask)

    # ---- per query: clause terms, exclusions, and the key of the call it can share ----
    groups: Dict[tuple, List[int]] = {}
    plans = []
    served = model.properties is not None
    from .history import DeviceHistory
    dh = history if isinstance(history, DeviceHistory) else None
    q_user_ids = dh.user_indices([q.get("user") for q in queries]) if dh is not None else None      # once per call: a keyed history resolves them on the device
    dated = served and ap.availableDateName is not None and ap.expireDateName is not None and ap.availableDateName in model.dates and ap.expireDateName in model.dates
    for n, q in enumerate(queries):
        user_bias = q.get("userBias", ap.userBias if ap.userBias is not None else 1.0)
        item_bias = q.get("itemBias", ap.itemBias if ap.itemBias is not None else 1.0)
        if not served:
            for key in ("fields", "dateRange"):
                if q.get(key):
                    raise NotImplementedError(f"query key {key!r} needs a model built with item properties")
            if user_bias < 0:
                raise NotImplementedError("negative userBias (user history as a filter) needs a model built with item properties ({} will do)")
            if item_bias < 0:
                raise NotImplementedError("negative itemBias (similar items as a filter) needs a model built with item properties ({} will do)")
        # ---- rules: key -> the query's row of the rule (ANY / NONE: columns; RANGE: (lo, hi)); the key names the matrix ----
        rules: Dict[tuple, object] = {}
        seen: Dict[tuple, int] = {}
        boosted = []
        for f in (q.get("fields") or []):
            name, bias = f["name"], float(f.get("bias", 1.0))
            prop = model.properties.get(name)
            cols = np.unique(np.array([prop.values[v] for v in f.get("values", []) if v in prop.values], np.int64)) if prop is not None else None
            kind = "boost" if bias > 0 else "any" if bias < 0 else "none"
            k = seen[(kind, name, bias)] = seen.get((kind, name, bias), -1) + 1
            if bias > 0:                                                                        # getBoostedMetadata :842-849
                if prop is not None:
                    boosted.append(((name, bias, k), cols))
            elif bias < 0:                                                                      # getFilteringMetadata :852-859
                rules[("any", name, k) if prop is not None else ("never", k)] = cols if prop is not None else np.zeros(0, np.int64)
            elif prop is not None:                                                              # getExcludingMetadata :862-869
                rules[("none", name, k)] = cols
        dr = q.get("dateRange")
        if dr and (dr.get("after") or dr.get("before")):                                        # getFilteringDateRange :877-915
            rules[("range", dr["name"])] = (_date_ms(dr["after"], "dateRange.after") + 1 if dr.get("after") else NO_VALUE,
                                            _date_ms(dr["before"], "dateRange.before") if dr.get("before") else OPEN_HI)
        elif dated:                                                                             # :916-948 -- only without a dateRange
            import time
            now = _date_ms(q["currentDate"], "currentDate") if q.get("currentDate") else int(now_ms) if now_ms is not None else int(time.time() * 1000)
            rules[("range", ap.availableDateName)] = (NO_VALUE, now + 1)
            rules[("range", ap.expireDateName, "expire")] = (now + 1, OPEN_HI)
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
        events = history.get(user, {}) if user is not None and dh is None else {}
        hist_key = None
        if dh is not None:                                                                      # the rows come from the device, per group (D17)
            hist_key = (tuple(ev for ev in q_events if ev in dh.types and (ev in model.by_name or ev in blacklist_events)), user_bias < 0)
            if user_bias < 0:
                rules.update({("hist", ev): None if ev in dh.types else np.zeros(0, np.int64) for ev in q_events if ev in model.by_name})
        for ev in (q_events if dh is None else ()):                                             # getBiasedRecentUserActions :795-839
            c = model.by_name.get(ev)
            if c is None:
                continue
            recent = list(reversed(events.get(ev, [])))[: max_items.get(ev, 100)]               # most recent first, capped, then distinct
            ids = [model.column_index(c, i) for i in dict.fromkeys(recent)]
            ids = np.unique(np.array([i for i in ids if i is not None], np.int64))
            if user_bias < 0:                                                                   # buildQueryMust :688-693: a filter per event, no should-clause
                rules[("hist", ev)] = ids
            else:
                terms[("user", ev)] = ids
        for ev in q_events:                                                                     # getExcludedItems :741-767
            if ev in blacklist_events:
                excl += [model.item_index(i) for i in events.get(ev, [])]
        excl += [model.item_index(i) for i in (q.get("blacklistItems") or [])]
        q_item = -1
        if item is not None:
            i = model.item_index(item)
            if i is not None and dev_items:                                                     # the rows come from the device, per group (D18)
                q_item = i
                if item_bias < 0:
                    rules.update({("sim", ev): None for ev in model_events})
            elif i is not None:                                                                 # getBiasedSimilarItems :770-792
                for ev in model_events:
                    c = model.by_name[ev]
                    ids = model.indicator_row(c, i)
                    if ids.size > max_query_events:
                        ids = ids[: max_query_events - 1]
                    if item_bias < 0:                                                           # :695-699
                        rules[("sim", ev)] = np.unique(ids.astype(np.int64))
                    else:
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
        for slot, cols in boosted:
            terms[("field",) + slot] = cols
        # a rule cannot be absent for one row of a call: queries share a call only when they carry the same rules and the same property clauses
        key = (_boost(user_bias), _boost(item_bias), _boost(set_bias), start + num, tuple(slot for slot, _ in boosted), tuple(rules), hist_key)
        groups.setdefault(key, []).append(n)
        plans.append((terms, np.unique(np.array([i for i in excl if i is not None], np.int64)), start, num, rules, q_user_ids[n] if dh is not None else -1,
                      user is not None, q_item))

    # ---- one call per group ----
    results: List[Optional[dict]] = [None] * len(queries)
    dev = model.sess.device
    empty = np.zeros(0, np.int64)
    for (ub, ib, sb, fetch, field_slots, rule_keys, hist_key), members in groups.items():
        hist_rows: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        excl = _csr([plans[n][1] for n in members], dev)
        if hist_key is not None and hist_key[0]:                                                # one history call for the group
            if len(hist_key[0]) > _lib.REC_MAX_CLAUSES:
                raise ValueError(f"a batch names {len(hist_key[0])} event types, more than the {_lib.REC_MAX_CLAUSES} one history call serves")
            specs = [(dh.types[ev].n_cols, max_items.get(ev, 100), ev in blacklist_events, dh.types[ev].idx_row_ptr, dh.types[ev].idx_pos, dh.types[ev].items,
                      dh.types[ev].times, dh.types[ev].col_map) for ev in hist_key[0]]
            q_users = torch.tensor([plans[n][5] for n in members], dtype=torch.int32).to(dev)
            rows, excl, _ = model.sess.history_rows(q_users, dh.n_users, specs, model.n_items, excl)
            hist_rows = {ev: r for ev, r in zip(hist_key[0], rows) if ev in model.by_name}
        item_dev: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        if dev_items and any(plans[n][7] >= 0 for n in members):                                # one item call for the group
            if len(model_events) > _lib.REC_MAX_CLAUSES:
                raise ValueError(f"the model has {len(model_events)} event types, more than the {_lib.REC_MAX_CLAUSES} one item call serves")
            q_items = torch.tensor([plans[n][7] for n in members], dtype=torch.int32).to(dev)
            rows, _ = model.sess.item_rows(q_items, [(model.by_name[ev].n_cols, max_query_events, model.by_name[ev].row_ptr, model.by_name[ev].col_idx)
                                                     for ev in model_events], n_items=model.n_items)
            item_dev = dict(zip(model_events, rows))
        slots = []                                                                              # the reference's order (:653): history, similar items, metadata, item set
        for kind, boost in (("user", ub), ("item", ib), ("field", None), ("set", sb)):
            if kind == "field":
                slots += [(("field",) + slot, model.properties[slot[0]], slot[1]) for slot in field_slots
                          if any(plans[n][0][("field",) + slot].size for n in members)]
                continue
            for ev in ([primary] if kind == "set" else model_events if kind == "item" else list(model.by_name)):
                if kind == "user" and dh is not None:
                    if ev in hist_rows and not hist_key[1] and any(plans[n][6] for n in members):
                        slots.append(((kind, ev), model.by_name[ev], boost))
                    continue
                if kind == "item" and dev_items:                                                # under itemBias < 0 the rows are ANY rules, not clauses
                    if ev in item_dev and ("sim", ev) not in rule_keys:
                        slots.append(((kind, ev), model.by_name[ev], boost))
                    continue
                if any(plans[n][0].get((kind, ev), empty).size for n in members):
                    slots.append(((kind, ev), model.by_name[ev], boost))
        if len(slots) > _lib.REC_MAX_CLAUSES:
            raise ValueError(f"a batch needs {len(slots)} clauses, more than the {_lib.REC_MAX_CLAUSES} one call serves")
        if len(rule_keys) > _lib.REC_MAX_RULES:
            raise ValueError(f"a batch needs {len(rule_keys)} rules, more than the {_lib.REC_MAX_RULES} one call serves")
        clauses = []
        weights = None if tw is None else [tw.get(c.name) for _, c, _ in slots]                 # the clause's matrix names its array
        for slot, c, boost in slots:
            qrp, qci = (hist_rows[slot[1]] if slot[0] == "user" and dh is not None else item_dev[slot[1]] if slot[0] == "item" and dev_items else
                        _csr([plans[n][0].get(slot, empty) for n in members], dev))
            clauses.append((c.n_cols, boost, c.col_ptr, c.row_idx, qrp, qci))
        rules = None
        if served:
            rules = []
            for rk in rule_keys:
                if rk[0] == "range":
                    value = model.dates.get(rk[1])
                    if value is None:                                                           # no item holds the property: nothing passes
                        value = model.dates[rk[1]] = torch.full((max(model.n_items, 1),), NO_VALUE, dtype=torch.int64, device=dev)
                    lo, hi = (torch.tensor([plans[n][4][rk][side] for n in members], dtype=torch.int64).to(dev) for side in (0, 1))
                    rules.append((_lib.RULE_RANGE, value, lo, hi))
                else:
                    m = model.properties[rk[1]] if rk[0] in ("any", "none") else model.by_name[rk[1]] if rk[0] in ("hist", "sim") else model.correlators[0]
                    qrp, qci = (hist_rows[rk[1]] if rk[0] == "hist" and rk[1] in hist_rows else item_dev[rk[1]] if rk[0] == "sim" and dev_items else
                                _csr([plans[n][4][rk] for n in members], dev))
                    rules.append((_lib.RULE_NONE if rk[0] == "none" else _lib.RULE_ANY, m.n_cols, m.row_ptr, m.col_idx, qrp, qci))
        count, idx, score, _ = model.sess.recommend(len(members), model.n_items, clauses, fetch, excl, mask_t, model.fill_order, flags, stats=False, rules=rules,
                                                    weights=weights)
        model.sess.synchronize()
        count, idx, score = count.cpu().numpy(), idx.cpu().numpy(), score.cpu().numpy()
        for r, n in enumerate(members):
            start, num = plans[n][2], plans[n][3]
            results[n] = {"itemScores": [{"item": model.item_name(int(idx[r, j])), "score": float(score[r, j])} for j in range(start, min(int(count[r]), start + num))]}
    return results


def similar_items(algo, model: DeviceModel, items=None, num: Optional[int] = None, item_bias: Optional[float] = None, return_self: Optional[bool] = None,
                  chunk: int = 65536, item_mask=None, now_ms: Optional[int] = None, term_weights=None):
    """The item-to-item table ("people who liked this also liked"): row n is what batch_predict answers to {"item": items[n]} -- the same items in the
    same order with the same scores -- as three device tensors (count int32 [n], idx int32 [n, num], score float64 [n, num]); entries behind count[n]
    are -1 / 0.0.  No Python work per item: the queries go `chunk` at a time through DeviceSession.item_rows (decision D18) and recommend, and no
    matrix comes back to the host.
    items: a sequence of item ids, a device int32 tensor of dense item ids, or None = every item of the model; an id the model does not know is served
    as batch_predict serves an unknown item (the backfill alone).  num, item_bias, return_self: default to the algorithm's num (20), itemBias (1.0),
    returnSelf (False).  item_bias > 0: one should-clause per event type of the model over the item's own indicator lists, boost = the bias;
    item_bias < 0: the lists are ANY rules instead (a model built with item properties, {} will do).  The query item is excluded unless return_self.
    Backfill, recsModel, item_mask, the available / expire date rule around now_ms and term_weights are those of batch_predict."""
    ap = algo.ap
    sess, dev = model.sess, model.sess.device
    tw = _term_weights(algo, model, term_weights)
    model_events = list(algo.modelEventNames)
    for ev in model_events:
        if ev not in model.by_name:
            raise ValueError(f"the model holds no indicator matrix for event {ev!r}")
    if len(model_events) > _lib.REC_MAX_CLAUSES:
        raise ValueError(f"the model has {len(model_events)} event types, more than the {_lib.REC_MAX_CLAUSES} one call serves")
    num = int(num if num is not None else ap.num if ap.num is not None else 20)
    if num < 1 or num > _lib.REC_MAX_NUM:
        raise ValueError(f"num must lie in 1..{_lib.REC_MAX_NUM}, got {num}")
    bias = float(item_bias if item_bias is not None else ap.itemBias if ap.itemBias is not None else 1.0)
    keep_self = bool(return_self if return_self is not None else ap.returnSelf if ap.returnSelf is not None else False)
    max_terms = _max_query_events(ap)
    if max_terms < 1 or chunk < 1:
        raise ValueError("similar_items needs maxQueryEvents >= 1 and chunk >= 1")
    served = model.properties is not None
    if bias < 0 and not served:
        raise NotImplementedError("negative itemBias (similar items as a filter) needs a model built with item properties ({} will do)")
    flags = _lib.REC_NO_BACKFILL if algo.recsModel == "collabFiltering" else 0
    mask_t = _mask_tensor(model, item_mask)
    if items is None:
        q_all = torch.arange(model.n_items, dtype=torch.int32, device=dev)
    elif torch.is_tensor(items):
        if items.dtype != torch.int32 or items.dim() != 1:
            raise ValueError("items as a tensor: dense item ids, int32, one dimension")
        q_all = items.to(dev)
    else:
        idx_of = [model.item_index(i) for i in items]
        q_all = torch.tensor([-1 if i is None else i for i in idx_of], dtype=torch.int32).to(dev)
    n = int(q_all.numel())
    dates = []
    if served and ap.availableDateName is not None and ap.expireDateName is not None and ap.availableDateName in model.dates and ap.expireDateName in model.dates:
        import time
        now = int(now_ms) if now_ms is not None else int(time.time() * 1000)
        dates = [(model.dates[ap.availableDateName], NO_VALUE, now + 1), (model.dates[ap.expireDateName], now + 1, OPEN_HI)]
    specs = [(model.by_name[ev].n_cols, max_terms, model.by_name[ev].row_ptr, model.by_name[ev].col_idx) for ev in model_events]
    count = torch.zeros(n, dtype=torch.int32, device=dev)
    idx = torch.full((n, num), -1, dtype=torch.int32, device=dev)
    score = torch.zeros((n, num), dtype=torch.float64, device=dev)
    for lo in range(0, n, chunk):
        q = q_all[lo:lo + chunk].contiguous()
        m = int(q.numel())
        known = (q >= 0) & (q < model.n_items)
        rows, _ = sess.item_rows(q, specs, n_items=model.n_items)
        if keep_self:
            excl = (torch.zeros(m + 1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
        else:                                                                                   # one exclusion per known query item: the item itself
            rp = torch.zeros(m + 1, dtype=torch.int64, device=dev)
            rp[1:] = torch.cumsum(known, 0)
            excl = (rp, torch.cat([q[known], torch.zeros(1, dtype=torch.int32, device=dev)]))
        rules = None
        if served:
            rules = [(_lib.RULE_RANGE, value, torch.full((m,), lo_ms, dtype=torch.int64, device=dev), torch.full((m,), hi_ms, dtype=torch.int64, device=dev))
                     for value, lo_ms, hi_ms in dates]
        if bias < 0:
            sim = [(_lib.RULE_ANY, model.by_name[ev].n_cols, model.by_name[ev].row_ptr, model.by_name[ev].col_idx, qrp, qci) for ev, (qrp, qci) in zip(model_events, rows)]
            c, i, s, _ = sess.recommend(m, model.n_items, [], num, excl, mask_t, model.fill_order, flags, stats=False, rules=sim + rules)
            if not bool(known.all()):                                                           # an unknown item carries no rule: the backfill alone
                c2, i2, s2, _ = sess.recommend(m, model.n_items, [], num, excl, mask_t, model.fill_order, flags, stats=False, rules=rules)
                c, i, s = torch.where(known, c, c2), torch.where(known[:, None], i, i2), torch.where(known[:, None], s, s2)
        else:
            clauses = [(model.by_name[ev].n_cols, _boost(bias), model.by_name[ev].col_ptr, model.by_name[ev].row_idx, qrp, qci) for ev, (qrp, qci) in zip(model_events, rows)]
            c, i, s, _ = sess.recommend(m, model.n_items, clauses, num, excl, mask_t, model.fill_order, flags, stats=False, rules=rules,
                                        weights=None if tw is None else [tw.get(ev) for ev in model_events])
        live = torch.arange(num, device=dev)[None, :] < c[:, None]
        count[lo:lo + m] = c
        idx[lo:lo + m] = torch.where(live, i, idx[lo:lo + m])
        score[lo:lo + m] = torch.where(live, s, score[lo:lo + m])
    return count, idx, score


def user_recommendations(algo, model: DeviceModel, history, users=None, num: Optional[int] = None, event_names: Optional[Sequence[str]] = None,
                         user_bias: Optional[float] = None, chunk: int = 65536, item_mask=None, now_ms: Optional[int] = None, term_weights=None):
    """The per-user table, the user-side twin of similar_items: row n is what batch_predict answers to {"user": users[n]} (with "eventNames", "num" and
    "userBias" where given) over the same DeviceHistory -- the same items in the same order with the same scores -- as three device tensors (count
    int32 [n], idx int32 [n, num], score float64 [n, num]); entries behind count[n] are -1 / 0.0.  No Python work per user: the queries go `chunk`
    at a time through DeviceSession.history_rows (decision D17) and recommend.
    history: a history.DeviceHistory.  users: None = every user id of the history, a device int32 tensor of dense user ids, or a sequence of users
    resolved with DeviceHistory.user_index; a user the history does not know (an id < 0 or >= n_users) is served as batch_predict serves one: the
    backfill alone, or nothing when the history is a filter.  num, user_bias: default to the algorithm's num (20) and userBias (1.0).  event_names:
    the query's `eventNames`, default the model's event types.  user_bias > 0: one should-clause per event type over the user's recent items, boost
    = the bias; user_bias < 0: the rows are ANY rules instead (a model built with item properties, {} will do) -- every query carries them, so an
    unknown user or an event without history matches nothing, as in batch_predict.  The blacklist events' exclusions, backfill, recsModel, item_mask
    the available / expire date rule around now_ms and term_weights are those of batch_predict."""
    from .history import DeviceHistory
    tw = _term_weights(algo, model, term_weights)
    if not isinstance(history, DeviceHistory):
        raise ValueError("user_recommendations needs a history.DeviceHistory (the event streams resident on the device)")
    dh = history
    ap = algo.ap
    sess, dev = model.sess, model.sess.device
    model_events = list(algo.modelEventNames)
    primary = model_events[0]
    for ev in model_events:
        if ev not in model.by_name:
            raise ValueError(f"the model holds no indicator matrix for event {ev!r}")
    num = int(num if num is not None else ap.num if ap.num is not None else 20)
    if num < 1 or num > _lib.REC_MAX_NUM:
        raise ValueError(f"num must lie in 1..{_lib.REC_MAX_NUM}, got {num}")
    if chunk < 1:
        raise ValueError("user_recommendations needs chunk >= 1")
    bias = float(user_bias if user_bias is not None else ap.userBias if ap.userBias is not None else 1.0)
    served = model.properties is not None
    if bias < 0 and not served:
        raise NotImplementedError("negative userBias (user history as a filter) needs a model built with item properties ({} will do)")
    max_items = {i.name: (i.maxItemsPerUser if i.maxItemsPerUser is not None else 500) for i in ap.indicators} if ap.indicators else {e: 100 for e in model_events}
    blacklist_events = ap.blacklistEvents if ap.blacklistEvents is not None else [primary]
    q_events = list(event_names or model_events)
    hist_events = [ev for ev in q_events if ev in dh.types and (ev in model.by_name or ev in blacklist_events)]
    if len(hist_events) > _lib.REC_MAX_CLAUSES:
        raise ValueError(f"a batch names {len(hist_events)} event types, more than the {_lib.REC_MAX_CLAUSES} one history call serves")
    flags = _lib.REC_NO_BACKFILL if algo.recsModel == "collabFiltering" else 0
    mask_t = _mask_tensor(model, item_mask)
    if users is None:
        q_all = torch.arange(dh.n_users, dtype=torch.int32, device=dev)
    elif torch.is_tensor(users):
        if users.dtype != torch.int32 or users.dim() != 1:
            raise ValueError("users as a tensor: dense user ids, int32, one dimension")
        q_all = users.to(dev)
    else:
        q_all = torch.tensor(dh.user_indices(users), dtype=torch.int32).to(dev)
    n = int(q_all.numel())
    dates = []
    if served and ap.availableDateName is not None and ap.expireDateName is not None and ap.availableDateName in model.dates and ap.expireDateName in model.dates:
        import time
        now = int(now_ms) if now_ms is not None else int(time.time() * 1000)
        dates = [(model.dates[ap.availableDateName], NO_VALUE, now + 1), (model.dates[ap.expireDateName], now + 1, OPEN_HI)]
    specs = [(dh.types[ev].n_cols, max_items.get(ev, 100), ev in blacklist_events, dh.types[ev].idx_row_ptr, dh.types[ev].idx_pos, dh.types[ev].items,
              dh.types[ev].times, dh.types[ev].col_map) for ev in hist_events]
    rule_events = list(dict.fromkeys(ev for ev in q_events if ev in model.by_name)) if bias < 0 else []
    if len(rule_events) + len(dates) > _lib.REC_MAX_RULES:
        raise ValueError(f"a batch needs {len(rule_events) + len(dates)} rules, more than the {_lib.REC_MAX_RULES} one call serves")
    count = torch.zeros(n, dtype=torch.int32, device=dev)
    idx = torch.full((n, num), -1, dtype=torch.int32, device=dev)
    score = torch.zeros((n, num), dtype=torch.float64, device=dev)
    for lo in range(0, n, chunk):
        q = q_all[lo:lo + chunk].contiguous()
        m = int(q.numel())
        none = (torch.zeros(m + 1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
        hist_rows: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        excl = none
        if specs:
            rows, excl, _ = sess.history_rows(q, dh.n_users, specs, model.n_items)
            hist_rows = {ev: r for ev, r in zip(hist_events, rows) if ev in model.by_name}
        rules = None
        if served:
            rules = [(_lib.RULE_RANGE, value, torch.full((m,), lo_ms, dtype=torch.int64, device=dev), torch.full((m,), hi_ms, dtype=torch.int64, device=dev))
                     for value, lo_ms, hi_ms in dates]
        clauses, weights = [], None
        if bias < 0:                                                                            # a filter per event, no should-clause; an event without history matches nothing
            rules = rules + [(_lib.RULE_ANY, model.by_name[ev].n_cols, model.by_name[ev].row_ptr, model.by_name[ev].col_idx) + hist_rows.get(ev, none) for ev in rule_events]
        else:                                                                                   # the clauses in the model's order, as batch_predict lays them out
            clauses = [(c.n_cols, _boost(bias), c.col_ptr, c.row_idx) + hist_rows[c.name] for c in model.correlators if c.name in hist_rows]
            weights = None if tw is None else [tw.get(c.name) for c in model.correlators if c.name in hist_rows]
        c, i, s, _ = sess.recommend(m, model.n_items, clauses, num, excl, mask_t, model.fill_order, flags, stats=False, rules=rules, weights=weights)
        live = torch.arange(num, device=dev)[None, :] < c[:, None]
        count[lo:lo + m] = c
        idx[lo:lo + m] = torch.where(live, i, idx[lo:lo + m])
        score[lo:lo + m] = torch.where(live, s, score[lo:lo + m])
    return count, idx, score
