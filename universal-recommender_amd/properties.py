"""The event store's view of the items, resident on the GPU (decision D25 of DESIGN.md; include/urcco.h urcco_dev_props_*).

What the reference reads with PEventStore.aggregateProperties(entityType = "item") (DataSource.scala:93-97) and indexes next to the indicators --
`DeviceModel.from_indicators(properties=...)` takes it as a dict that is already aggregated, once -- a DeviceProperties holds as the property events
themselves: per property name one stream of $set / $unset events (item, time, and per $set the value) with the aggregation state, and the $delete
events' state.  New events are aggregated on the device where they arrive (`apply`), and `materialise` cuts the item x value matrices, the date arrays
and `item_mask` the "deleted" mask of a serving model from the state: `model.set_properties(props)` installs them without touching the indicators.

The rule (include/urcco.h states the contract): a property of an item is alive when its latest $set -- by (time, stream position) -- is later than the
latest $unset of the key and the latest $delete of the item, a tie going to the $unset / $delete; its value is that $set's alone; an item is deleted when
it has a $delete that no $set of any of its keys is later than.  The rule does not depend on the order or the batching of the events.

Served: list-of-strings properties (rule matrices) and the properties in `date_names` (ISO-8601 strings through URModel.extractJvalue, as
`_device_properties` parses them); `compact` takes the superseded values out of the value streams (decision D28), when the caller says so.  Not
served: merging list values across sets, properties of any other type (ignored, as `_device_properties` ignores them), items outside the primary's dictionary (ignored), the JVM
seam, the multi-GPU build."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .device import DevCsr, DeviceSession
from .history import GROWTH
from .recommend import NO_VALUE, _Property


@dataclass
class _PropStream:
    """One property: the $set / $unset stream in buffers with spare capacity (the first n_events / n_values entries are live) and its state."""
    name: str
    is_date: bool
    t_set: torch.Tensor                      # int64 [n_items]: the bits of the header's uint64 words
    pos_set: torch.Tensor                    # int32 [n_items]
    t_unset: torch.Tensor                    # int64 [n_items]
    n_events: int = 0
    n_values: int = 0
    items: Optional[torch.Tensor] = None     # int32
    times: Optional[torch.Tensor] = None     # int64
    kinds: Optional[torch.Tensor] = None     # uint8
    val_ptr: Optional[torch.Tensor] = None   # lists: int64 [n_events + 1]
    vals: Optional[torch.Tensor] = None      # lists: int32 [n_values] value ids
    date_vals: Optional[torch.Tensor] = None  # dates: int64 [n_events] epoch milliseconds
    values: Dict[str, int] = field(default_factory=dict)   # lists: value -> column, grows as new values appear


class DeviceProperties:
    """Item property events by item in HBM, for the items of `model`'s primary dictionary."""

    def __init__(self, sess: DeviceSession, model, date_names: Sequence[str] = ()):
        self.sess, self.model, self.date_names = sess, model, list(date_names)
        self.n_items = int(model.n_items)
        self.streams: Dict[str, _PropStream] = {}
        self.t_del = self._zeros(self.n_items, torch.int64)
        self.last_compact: Dict[str, Tuple[int, int, int, int]] = {}   # `compact`: name -> (events before, after, values before, after) of the last call

    # ---- buffers ----
    def _zeros(self, n: int, dtype) -> torch.Tensor:
        t = self.sess.empty(max(n, 1), dtype)
        t.zero_()
        return t

    def _grown(self, buf: Optional[torch.Tensor], n_live: int, need: int, dtype) -> torch.Tensor:
        """A buffer of at least `need` entries that keeps the first n_live of `buf`: `buf` when it is large enough, else a new one, GROWTH times larger
        (DeviceHistory._grown's rule)."""
        if buf is not None and buf.numel() >= need:
            return buf
        new = self.sess.empty(max(need, GROWTH * (buf.numel() if buf is not None else 0), 1), dtype)
        if n_live:
            new[:n_live].copy_(buf[:n_live])
        return new

    def _stream(self, name: str) -> _PropStream:
        s = self.streams.get(name)
        if s is None:
            s = self.streams[name] = _PropStream(name, name in self.date_names, self._zeros(self.n_items, torch.int64), self._zeros(self.n_items, torch.int32),
                                                 self._zeros(self.n_items, torch.int64))
            if not s.is_date:
                s.val_ptr = self._zeros(1, torch.int64)
        return s

    def grow(self, n_items: int) -> "DeviceProperties":
        """The catalogue grew to n_items: every state array is extended by zeros ("nothing seen"); returns self."""
        n_items = int(n_items)
        if n_items < self.n_items:
            raise ValueError("the item id space does not shrink")

        def ext(t):
            new = self._zeros(n_items, t.dtype)
            new[: self.n_items].copy_(t[: self.n_items])
            return new
        self.t_del = ext(self.t_del)
        for s in self.streams.values():
            s.t_set, s.pos_set, s.t_unset = ext(s.t_set), ext(s.pos_set), ext(s.t_unset)
        self.n_items = n_items
        return self

    def _dev(self, a, dtype) -> torch.Tensor:
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if t.dtype != dtype:
            raise ValueError(f"{dtype} expected, got {t.dtype}")
        return t.to(self.sess.device).contiguous()

    # ---- events ----
    def apply_streams(self, streams: Dict[str, tuple], deletes: Optional[tuple] = None, new_values: Optional[Dict[str, Sequence[str]]] = None) -> "DeviceProperties":
        """New events in dense-id tensor form, aggregated in place; returns self.  streams: property name -> (items int32, times int64, kinds uint8 | None,
        payload): for a list property payload = (val_ptr int64 [n + 1] starting at 0, value ids int32) -- the value slice of every event, an $unset's empty
        -- for a name in date_names payload = int64 [n] epoch milliseconds (an $unset's entry is not read).  kinds: _lib.PROP_SET / PROP_UNSET per event,
        None = all sets.  deletes: (items int32, times int64) of the $delete events.  new_values: property name -> value strings appended to its
        dictionary (a value id beyond the dictionary has no column and is dropped).  Tensors or numpy arrays, on any device.  Events with time INT64_MIN
        and items outside 0 .. n_items are ignored.  Does not synchronise."""
        for name, vals in (new_values or {}).items():
            d = self._stream(name).values
            for v in vals:
                d.setdefault(v, len(d))
        for name, (items, times, kinds, payload) in streams.items():
            s = self._stream(name)
            items, times = self._dev(items, torch.int32), self._dev(times, torch.int64)
            n = int(items.numel())
            if times.numel() != n or (kinds is not None and len(kinds) != n):
                raise ValueError(f"property {name!r}: items, times and kinds of one length expected")
            if n == 0:
                continue
            old, need = s.n_events, s.n_events + n
            if need >= (1 << 31):
                raise ValueError(f"property {name!r}: a stream holds fewer than 2^31 events")
            s.items, s.times = self._grown(s.items, old, need, torch.int32), self._grown(s.times, old, need, torch.int64)
            s.kinds = self._grown(s.kinds, old, need, torch.uint8)
            s.items[old:need].copy_(items)
            s.times[old:need].copy_(times)
            if kinds is None:
                s.kinds[old:need].fill_(_lib.PROP_SET)
            else:
                s.kinds[old:need].copy_(self._dev(kinds, torch.uint8))
            if s.is_date:
                s.date_vals = self._grown(s.date_vals, old, need, torch.int64)
                s.date_vals[old:need].copy_(self._dev(payload, torch.int64))
            else:
                vp, vals = self._dev(payload[0], torch.int64), self._dev(payload[1], torch.int32)
                if vp.numel() != n + 1:
                    raise ValueError(f"property {name!r}: val_ptr holds one entry per event and the total")
                nv = int(vals.numel())
                s.val_ptr = self._grown(s.val_ptr, old + 1, need + 1, torch.int64)
                s.val_ptr[old + 1: need + 1].copy_(vp[1:] + s.n_values)
                s.vals = self._grown(s.vals, s.n_values, s.n_values + nv, torch.int32)
                if nv:
                    s.vals[s.n_values: s.n_values + nv].copy_(vals)
                s.n_values += nv
            self.sess.props_apply(self.n_items, s.items[old:need], s.times[old:need], s.kinds[old:need], old, s.t_set, s.pos_set, s.t_unset)
            s.n_events = need
        if deletes is not None:
            items, times = self._dev(deletes[0], torch.int32), self._dev(deletes[1], torch.int64)
            if items.numel() != times.numel():
                raise ValueError("deletes: items and times of one length expected")
            if items.numel():
                self.sess.props_delete(self.n_items, items, times, self.t_del)
        return self

    def apply(self, events) -> "DeviceProperties":
        """New property events, aggregated in place; returns self.  An event is (item, "$set" | "$unset" | "$delete", {name: value} | [names] | None,
        time_ms): a $set carries the properties it sets, an $unset the names it removes (a dict's keys count), a $delete nothing.  One event is split per
        key into the per-property streams, every part at the event's time.  Ignored: items outside the primary's dictionary; in a $set, a value that is
        neither a list of strings nor, for a name in date_names, a string (URModel.extractJvalue parses it)."""
        from .ur_model import extractJvalue
        parts: Dict[str, list] = {}
        d_items: List[int] = []
        d_times: List[int] = []
        new_values: Dict[str, List[str]] = {}
        for item, kind, props, time_ms in events:
            i = self.model.item_index(item)
            if i is None or not 0 <= i < self.n_items:
                continue
            t = int(time_ms)
            if kind == "$delete":
                d_items.append(i)
                d_times.append(t)
            elif kind == "$unset":
                for name in (props or ()):
                    parts.setdefault(name, []).append((i, t, _lib.PROP_UNSET, None))
            elif kind == "$set":
                for name, value in (props or {}).items():
                    if name in self.date_names:
                        if isinstance(value, str):
                            ms = int(round(extractJvalue(self.date_names, name, value).timestamp() * 1000))
                            parts.setdefault(name, []).append((i, t, _lib.PROP_SET, ms))
                    elif isinstance(value, (list, tuple)) and all(isinstance(v, str) for v in value):
                        d = self._stream(name).values
                        new = new_values.setdefault(name, [])
                        ids = []
                        for v in value:
                            if v not in d:
                                d[v] = len(d)
                                new.append(v)
                            ids.append(d[v])
                        parts.setdefault(name, []).append((i, t, _lib.PROP_SET, ids))
            else:
                raise ValueError(f"property event {kind!r}: $set, $unset or $delete expected")
        streams = {}
        for name, evs in parts.items():
            items = np.array([e[0] for e in evs], np.int32)
            times = np.array([e[1] for e in evs], np.int64)
            kinds = np.array([e[2] for e in evs], np.uint8)
            if name in self.date_names:
                payload = np.array([e[3] if e[3] is not None else NO_VALUE for e in evs], np.int64)
            else:
                lens = [len(e[3]) if e[3] is not None else 0 for e in evs]
                vp = np.zeros(len(evs) + 1, np.int64)
                np.cumsum(lens, out=vp[1:])
                payload = (vp, np.array([v for e in evs if e[3] for v in e[3]], np.int32))
            streams[name] = (items, times, kinds, payload)
        return self.apply_streams(streams, (np.array(d_items, np.int32), np.array(d_times, np.int64)) if d_items else None)

    @staticmethod
    def from_property_map(sess: DeviceSession, model, properties, date_names: Sequence[str] = (), time_ms: int = 0) -> "DeviceProperties":
        """An aggregated dict item -> {name: value} (URModel.propertiesMaps[0], what from_indicators(properties=...) takes) as $set events at one time."""
        return DeviceProperties(sess, model, date_names).apply((item, "$set", fields, time_ms) for item, fields in properties.items())

    # ---- what a model reads ----
    def _state(self, s: _PropStream):
        return (s.t_set, s.pos_set, s.t_unset, self.t_del, s.n_events)

    def materialise(self) -> Tuple[Dict[str, _Property], Dict[str, torch.Tensor]]:
        """(properties, dates) in the form DeviceModel holds them: per list property with at least one value the item x value matrix (CSR from
        urcco_dev_props_rows, CSC from the column counts and the transposition), per name of date_names the int64 array, NO_VALUE where the item has no
        date.  Reads, per list property, the bound total and the number of entries: two synchronisations each."""
        sess, n = self.sess, self.n_items
        props: Dict[str, _Property] = {}
        for name, s in self.streams.items():
            if s.is_date or not s.values:
                continue
            n_cols = len(s.values)
            vals = s.vals if s.vals is not None else sess.empty(1, torch.int32)
            rp, ci, _ = sess.props_rows(n, self._state(s), s.val_ptr, vals, s.n_values, n_cols)
            nnz = int(rp[n].item())
            ci = ci[:nnz]
            counts = sess.column_counts(ci, nnz, n_cols, sess.empty(n_cols, torch.int32))
            cp, ri = sess.transpose(DevCsr(n, n_cols, rp, ci, nnz), counts)
            props[name] = _Property(name, n_cols, dict(s.values), rp, ci, cp, ri)
        dates: Dict[str, torch.Tensor] = {}
        for name in self.date_names:
            s = self.streams.get(name)
            if s is None or s.n_events == 0:
                dates[name] = torch.full((n,), NO_VALUE, dtype=torch.int64).to(sess.device)
            else:
                dates[name] = sess.props_dates(n, self._state(s), s.date_vals)
        return props, dates

    def compact(self, names: Optional[Sequence[str]] = None) -> "DeviceProperties":
        """The streams of the properties `names` (default: all) without the events no item's state names any more (decision D28 of DESIGN.md;
        include/urcco.h urcco_dev_props_compact); returns self.  Of every item the winning $set's position stays -- with an empty value slice where the
        property is not alive: a maximum only grows, it cannot live again -- and the positions keep their order, so `apply`, `apply_streams`,
        `materialise`, `item_mask` and `grow` work on as before and give, bit for bit, what they would have given without the call.  The outputs become the
        buffers, with the capacity the old ones had: their tail is the spare capacity the next `apply` fills.  One device-to-host read, of the counts
        of all properties together.  `last_compact` = {name: (events before, events after, values before, values after)}.  No automatic trigger: the
        caller decides when, as with DeviceHistory.trim.  ValueError -- nothing is modified: a name the store does not hold."""
        todo = list(self.streams) if names is None else list(names)
        for name in todo:
            if name not in self.streams:
                raise ValueError(f"compact: the store holds no property {name!r}")
        sess = self.sess
        calls = []
        for name in todo:      # every call first, then the one read of the counts; the store changes only after both
            s = self.streams[name]
            if s.n_events == 0:
                continue
            if s.is_date:
                out = (None, None, sess.empty(s.date_vals.numel(), torch.int64))
                r = sess.props_compact(self.n_items, self._state(s), date_values=s.date_vals, out=out)
            else:
                vals = s.vals if s.vals is not None else sess.empty(1, torch.int32)
                out = (sess.empty(s.val_ptr.numel(), torch.int64), sess.empty(vals.numel(), torch.int32), None)
                r = sess.props_compact(self.n_items, self._state(s), s.val_ptr, vals, s.n_values, out=out)
            calls.append((s, r))
        counts = torch.stack([r[5] for _, r in calls]).cpu().tolist() if calls else []
        self.last_compact = {name: (self.streams[name].n_events, self.streams[name].n_events, self.streams[name].n_values, self.streams[name].n_values) for name in todo}
        for (s, (pos_set, old_pos, o_vp, o_vals, o_dates, _)), (k, v) in zip(calls, counts):
            k, v = int(k), int(v)
            self.last_compact[s.name] = (s.n_events, k, s.n_values, v)
            order = old_pos[:k].long()
            for attr in ("items", "times", "kinds"):      # the streams' own arrays follow the positions: n_events stays the length of every one
                buf = getattr(s, attr)
                new = sess.empty(buf.numel(), buf.dtype)
                if k:
                    new[:k].copy_(buf[order])
                setattr(s, attr, new)
            s.pos_set = pos_set
            if s.is_date:
                s.date_vals = o_dates
            else:
                s.val_ptr, s.vals = o_vp, o_vals
            s.n_events, s.n_values = k, v
        return self

    def item_mask(self) -> torch.Tensor:
        """uint8 [n_items] on the device: 0 where the item is deleted, else 1 -- the item_mask of batch_predict.  Does not synchronise."""
        t_sets = [s.t_set for s in self.streams.values()]
        mask = None
        for k in range(0, max(len(t_sets), 1), _lib.PROP_MAX):     # deleted = no later set in ANY chunk: the chunks' masks combine by maximum
            m = self.sess.props_exists(self.n_items, self.t_del, t_sets[k: k + _lib.PROP_MAX])
            mask = m if mask is None else torch.maximum(mask, m)
        return mask
