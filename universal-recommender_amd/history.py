"""The event store's view of the users, resident on the GPU (decision D17 of DESIGN.md; include/urcco.h urcco_dev_history_*).

What the reference fetches from the event store per query -- the most recent maxItemsPerUser events per event type, then distinct
(getBiasedRecentUserActions, URAlgorithm.scala:795-839), and every item of the user's blacklist events (getExcludedItems, :741-767) --
batch_predict otherwise computes in Python, per query, from a dict user -> {event: [items]}.  A DeviceHistory holds the event streams
themselves ((user id, column id, time) per event and event type, as the device ingest leaves them) with an index by user, and
`recommend.batch_predict(..., history=<DeviceHistory>)` builds the term rows and the exclusion rows of a whole group of queries with one
urcco_dev_history_bounds + urcco_dev_history_rows call.

The user ids of a history are its OWN dense ids; they need not be the user dictionary of the model build: the reference's event store
also knows users that `minEventsPerUser` dropped from the model, and their history is used all the same.

Recency is (time desc, stream position desc): of two events with equal time the later one in the stream is the more recent (the reference
leaves such ties to the event store).  Events whose item lies outside the event type's column dictionary (id -1) count toward the cap but
give no term, as in the dict form; as exclusions they are dropped, where the dict form still excludes such an item if the primary event
knows it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .device import DeviceSession


@dataclass
class _Stream:
    n_cols: int
    idx_row_ptr: torch.Tensor          # int64 [n_users + 1]: DeviceSession.history_index of the stream's user ids
    idx_pos: torch.Tensor              # int32 [n_events]
    items: torch.Tensor                # int32 [n_events]: column id of the event type (primary item id for an event outside the model), < 0 = none
    times: Optional[torch.Tensor]      # int64 [n_events] epoch milliseconds; None: stream order is time order
    col_map: Optional[torch.Tensor]    # int32 [n_cols] -> primary item id or -1; None: identity


class DeviceHistory:
    """Event streams by user in HBM.  `types[event name]` = the stream of that event type; an event name outside the model may be present
    (it can only feed exclusions: blacklistEvents), its column ids are then the primary's item ids."""

    def __init__(self, sess: DeviceSession, n_users: int, user_ids, types: Dict[str, _Stream]):
        self.sess, self.n_users, self.user_ids, self.types = sess, int(n_users), user_ids, types

    def user_index(self, user) -> int:
        """Dense id of a query's user, -1 when the history does not know it."""
        if user is None:
            return -1
        if self.user_ids is not None:
            i = self.user_ids.get(user)
            return -1 if i is None else int(i)
        try:
            i = int(user)
        except (TypeError, ValueError):
            return -1
        return i if 0 <= i < self.n_users else -1

    @staticmethod
    def _col_map(sess: DeviceSession, model, ev: str) -> Tuple[int, Optional[torch.Tensor]]:
        c = model.by_name.get(ev)
        if c is None:
            return model.n_items, None
        if c.column_ids is None or model.item_ids is None:
            return c.n_cols, None                      # dense integers on both sides: the same id space
        m = np.array([model.item_ids.getOrElse(c.column_ids.inverse(j), -1) for j in range(c.n_cols)], np.int32)
        if np.array_equal(m, np.arange(c.n_cols)):
            return c.n_cols, None
        return c.n_cols, torch.from_numpy(m if m.size else np.zeros(1, np.int32)).to(sess.device)

    @staticmethod
    def from_streams(sess: DeviceSession, model, streams: Dict[str, Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]], user_ids=None,
                     n_users: Optional[int] = None) -> "DeviceHistory":
        """streams: event name -> (user ids int32, item ids int32, times int64 | None), device tensors of one length per event type.  The ids are
        dense: user ids of ONE id space shared by all streams (user_ids: a BiDictionary / dict user -> id that batch_predict resolves query users
        with; None: queries name users by their integer id), item ids in the column dictionary of the event type, as
        `dictionary_lookup` yields them (-1: not in it).  n_users: the size of the user id space (default: len(user_ids), else the largest id + 1
        -- one synchronisation).  The column maps to the model's primary item dictionary come from the model's BiDictionaries, identity without."""
        if n_users is None:
            n_users = len(user_ids) if user_ids is not None else max([int(u.max().item()) + 1 for u, _, _ in streams.values() if u.numel()] + [0])
        types = {}
        for ev, (users, items, times) in streams.items():
            if users.dtype != torch.int32 or items.dtype != torch.int32 or users.numel() != items.numel():
                raise ValueError(f"stream {ev!r}: int32 user ids and item ids of one length expected")
            if times is not None and (times.dtype != torch.int64 or times.numel() != users.numel()):
                raise ValueError(f"stream {ev!r}: int64 times, one per event, expected")
            n_cols, col_map = DeviceHistory._col_map(sess, model, ev)
            rp, pos = sess.history_index(users, n_users)
            types[ev] = _Stream(n_cols, rp, pos, items if items.numel() else sess.empty(1, torch.int32), times, col_map)
        return DeviceHistory(sess, n_users, user_ids, types)

    @staticmethod
    def from_dict(sess: DeviceSession, model, history: Dict[str, Dict[str, List[str]]]) -> "DeviceHistory":
        """The dict form of batch_predict's `history` (user -> {event name: [item ids, oldest first]}) loaded onto the device: every user gets a
        dense id, the list order is the time order, an item outside the event's column dictionary gets the id -1."""
        user_ids = {u: i for i, u in enumerate(history)}
        names: List[str] = []
        for events in history.values():
            names += [ev for ev in events if ev not in names]
        streams = {}
        for ev in names:
            c = model.by_name.get(ev)
            users: List[int] = []
            items: List[int] = []
            for u, events in history.items():
                ids = [(model.column_index(c, i) if c is not None else model.item_index(i)) for i in events.get(ev, [])]
                items += [-1 if i is None else i for i in ids]
                users += [user_ids[u]] * len(ids)
            streams[ev] = (torch.tensor(users, dtype=torch.int32).to(sess.device), torch.tensor(items, dtype=torch.int32).to(sess.device), None)
        return DeviceHistory.from_streams(sess, model, streams, user_ids)
