"""The event store's view of the users, resident on the GPU (decision D17 of DESIGN.md; include/urcco.h urcco_dev_history_*).

What the reference fetches from the event store per query -- the most recent maxItemsPerUser events per event type, then distinct
(getBiasedRecentUserActions, URAlgorithm.scala:795-839), and every item of the user's blacklist events (getExcludedItems, :741-767) --
batch_predict otherwise computes in Python, per query, from a dict user -> {event: [items]}.  A DeviceHistory holds the event streams
themselves ((user id, column id, time) per event and event type, as the device ingest leaves them) with an index by user, and
`recommend.batch_predict(..., history=<DeviceHistory>)` builds the term rows and the exclusion rows of a whole group of queries with one
urcco_dev_history_bounds + urcco_dev_history_rows call.

The user ids of a history are its OWN dense ids; they need not be the user dictionary of the model build: the reference's event store
also knows users that `minEventsPerUser` dropped from the model, and their history is used all the same.  A KEYED history (from_key_streams, decision
D26) numbers them itself: events name their users by 64-bit key, one growable device dictionary hands out the ids, and no host dict is kept.

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
    n_events: int = -1                 # events of the stream; -1: not stated (an empty stream holds one placeholder entry, so items.numel() does not say) -- append refuses
    # DeviceHistory.append: the tensors above are exact-length views of these buffers (None: the tensor is its own buffer, no spare capacity)
    items_buf: Optional[torch.Tensor] = None
    times_buf: Optional[torch.Tensor] = None
    idx_buf: Optional[Tuple[torch.Tensor, torch.Tensor]] = None     # (row_ptr, pos) the index lives in
    idx_spare: Optional[Tuple[torch.Tensor, torch.Tensor]] = None   # the pair the next merge writes into: the index of before the last append


GROWTH = 2     # DeviceHistory.append: a buffer that is too small is replaced by one of max(needed, GROWTH * its capacity) entries


class DeviceHistory:
    """Event streams by user in HBM.  `types[event name]` = the stream of that event type; an event name outside the model may be present
    (it can only feed exclusions: blacklistEvents), its column ids are then the primary's item ids.  A history built by from_streams / from_dict keeps a
    reference to the model (`model`): `append` takes the columns of an event name it does not hold yet from it."""

    def __init__(self, sess: DeviceSession, n_users: int, user_ids, types: Dict[str, _Stream], model=None):
        self.sess, self.n_users, self.user_ids, self.types = sess, int(n_users), user_ids, types
        self.model = model     # the model the column maps came from: `append` needs it for an event name the history does not hold yet
        self.last_trim: Dict[str, Tuple[int, int]] = {}     # `trim`: event -> (events before, events after) of the last call
        self.user_dict = None      # a keyed history (from_key_streams): the growable ingest.DevDictionary user key -> dense id; user_ids is then None
        self.check = False         # ... whose streams carry the users' check keys as a fourth entry

    def user_index(self, user) -> int:
        """Dense id of a query's user, -1 when the history does not know it."""
        if user is None:
            return -1
        if self.user_dict is not None:
            return self.user_indices([user])[0]
        if self.user_ids is not None:
            i = self.user_ids.get(user)
            return -1 if i is None else int(i)
        try:
            i = int(user)
        except (TypeError, ValueError):
            return -1
        return i if 0 <= i < self.n_users else -1

    def user_indices(self, users) -> List[int]:
        """user_index for a whole batch of query users.  A keyed history hashes the users' strings once (preparator.hash_keys of str(user), the keys
        from_key_streams was fed), looks them up in its user dictionary with one call and copies the ids to the host once: no synchronisation per user.
        A user the shared dictionary already knows but this history has not reached yet (an id >= n_users) is unknown, -1."""
        users = list(users)
        if self.user_dict is None:
            return [self.user_index(u) for u in users]
        named = [n for n, u in enumerate(users) if u is not None]
        out = [-1] * len(users)
        if named:
            from . import ingest
            from .preparator import hash_keys
            keys = torch.from_numpy(hash_keys([str(users[n]) for n in named], library=self.sess.lib)).to(self.sess.device)
            for n, i in zip(named, ingest.dictionary_lookup(self.sess, self.user_dict, keys).cpu().tolist()):
                out[n] = i if i < self.n_users else -1
        return out

    @staticmethod
    def from_key_streams(sess: DeviceSession, model, streams: Dict[str, tuple], check: bool = False, user_dict=None) -> "DeviceHistory":
        """A history whose users are named by 64-bit keys (decision D26 of DESIGN.md): streams = event name -> (user keys int64, items, times int64 | None),
        device tensors of one length per event type.  The user keys are preparator.hash_keys of the users' id strings; ONE growable device dictionary,
        shared by all event types, gives them their dense ids in order of first appearance -- the event types in the order the dict lists them -- and
        queries that name a user by its string are resolved through it (user_indices).  items: int32 dense column ids as from_streams takes them, or
        int64 keys (hash_keys of the items' id strings) looked up in model.key_dictionary(event): a key outside the catalogue gives -1, an event that
        counts toward the cap and gives no term.  New ITEMS are not served: the model's column spaces are sized by the catalogue.
        check: every stream carries the users' check keys (hash_keys with preparator.CHECK_SEED) as a fourth entry; ingest.HashCollision when two user
        strings share a key (the state it leaves: ingest.DevDictionary.extend).  user_dict: an ingest.DevDictionary to share -- the training and the
        held-out history of evaluate are built over one; default a new, empty one.  `append_keys` adds events, and users, later."""
        from . import ingest
        dh = DeviceHistory(sess, 0, None, {}, model)
        dh.user_dict = user_dict if user_dict is not None else ingest.dictionary_build(sess, sess.empty(0, torch.int64))
        dh.check = bool(check)
        return dh.append_keys(streams)

    def append_keys(self, streams: Dict[str, tuple]) -> "DeviceHistory":
        """`append` for a keyed history: streams as from_key_streams takes them, the event types with new events only.  Per event type, in the order the
        dict lists them, one ingest.DevDictionary.extend resolves the batch's users on the device -- a user not seen before gets the next id -- and the
        existing `append` merges the dense streams; n_users grows to the dictionary's n_ids (an empty dict brings a history level with a dictionary that
        another history has extended).  No host work per event or per user.
        ValueError -- nothing is modified: not a keyed history; a stream's tensors do not fit; what `append` refuses."""
        from . import ingest
        if self.user_dict is None:
            raise ValueError("append_keys needs a keyed history (DeviceHistory.from_key_streams)")
        for ev, tup in streams.items():      # everything `append` would refuse, before the dictionary grows
            if len(tup) != (4 if self.check else 3):
                raise ValueError(f"stream {ev!r}: (user keys, items, times{', user check keys' if self.check else ''}) expected")
            keys, items, times = tup[:3]
            if keys.dtype != torch.int64 or items.dtype not in (torch.int32, torch.int64) or keys.numel() != items.numel():
                raise ValueError(f"stream {ev!r}: int64 user keys and int32 item ids or int64 item keys of one length expected")
            if self.check and (tup[3].dtype != torch.int64 or tup[3].numel() != keys.numel()):
                raise ValueError(f"stream {ev!r}: int64 check keys, one per event, expected")
            if times is not None and (times.dtype != torch.int64 or times.numel() != keys.numel()):
                raise ValueError(f"stream {ev!r}: int64 times, one per event, expected")
            if items.dtype == torch.int64 and self.model is None:
                raise ValueError(f"stream {ev!r}: item keys need the model whose catalogue they are looked up in")
            st = self.types.get(ev)
            if st is None and self.model is None:
                raise ValueError(f"stream {ev!r}: the history does not hold this event type and was built without a model to take its columns from")
            if st is not None and (times is None) != (st.times is None):
                raise ValueError(f"stream {ev!r}: the stream {'has no times' if st.times is None else 'has times'}, the batch must agree")
            if st is not None and st.n_events < 0:
                raise ValueError(f"stream {ev!r}: built without its number of events (_Stream.n_events)")
        dense = {}
        for ev, tup in streams.items():
            keys, items, times = tup[:3]
            if items.dtype == torch.int64:
                items = ingest.dictionary_lookup(self.sess, self.model.key_dictionary(ev), items)
            users, _ = self.user_dict.extend(keys, check_keys=tup[3] if self.check else None)
            dense[ev] = (users, items, times)
        return self.append(dense, n_users=self.user_dict.n_ids)

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
            DeviceHistory._check_stream(ev, users, items, times)
            n_cols, col_map = DeviceHistory._col_map(sess, model, ev)
            rp, pos = sess.history_index(users, n_users)
            types[ev] = _Stream(n_cols, rp, pos, items if items.numel() else sess.empty(1, torch.int32), times, col_map, n_events=int(items.numel()))
        return DeviceHistory(sess, n_users, user_ids, types, model)

    @staticmethod
    def _check_stream(ev: str, users: torch.Tensor, items: torch.Tensor, times: Optional[torch.Tensor]):
        if users.dtype != torch.int32 or items.dtype != torch.int32 or users.numel() != items.numel():
            raise ValueError(f"stream {ev!r}: int32 user ids and item ids of one length expected")
        if times is not None and (times.dtype != torch.int64 or times.numel() != users.numel()):
            raise ValueError(f"stream {ev!r}: int64 times, one per event, expected")

    def _grown(self, buf: Optional[torch.Tensor], live: Optional[torch.Tensor], n_live: int, need: int, dtype) -> torch.Tensor:
        """A buffer of at least `need` entries whose first n_live are those of `live`: `buf` when it is large enough, else a new one, GROWTH times larger."""
        if buf is None:
            buf = live
        if buf is not None and buf.numel() >= need:
            return buf
        new = self.sess.empty(max(need, GROWTH * (buf.numel() if buf is not None else 0), 1), dtype)
        if n_live:
            new[:n_live].copy_(live[:n_live])
        return new

    def append(self, streams: Dict[str, Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]], user_ids=None, n_users: Optional[int] = None,
               model=None) -> "DeviceHistory":
        """New events behind the streams, in place (decision D21 of DESIGN.md; include/urcco.h urcco_dev_history_append); returns self.  streams: as
        from_streams takes them, the event types with new events only; per type the items (and the times, iff the stream has times) are appended to
        the stream and the index is replaced by the merge of the old index with the batch -- no index rebuild, and the user ids of the events
        already held are not needed.  Every result afterwards is the one of from_streams over the concatenated streams with the final n_users.

        n_users may grow, never shrink: default len(user_ids) when a new `user_ids` is given (it replaces the old one), else the larger of the old
        size and the batch's largest id + 1 (one synchronisation, as in from_streams).  When it grows, the event types without new events get their
        index extended; a type for which nothing changes costs no call.  An event name the history does not hold yet is added as from_streams adds
        it (model: default the one the history was built from).

        Memory: the stream tensors and the index live in buffers with spare capacity; one that is too small is replaced by one GROWTH (2) times
        larger, so the cost of an append is the merge (one copy of the old index plus the batch), not a reallocation of the streams.  _Stream.items
        / .times / .idx_* stay exact-length views.  The merge cannot run in place: every event type that was appended to keeps a second index
        buffer, the one the next merge writes into.

        ValueError -- nothing is modified before all streams passed: dtypes or lengths as in from_streams; times given for a stream that has none or
        missing for one that has them; a shrinking n_users; a new event name without a model; a _Stream built by hand without n_events."""
        model = model if model is not None else self.model
        new_cols = {}      # the columns of the event names the history does not hold yet, resolved before anything is modified
        for ev, (users, items, times) in streams.items():
            self._check_stream(ev, users, items, times)
            st = self.types.get(ev)
            if st is None:
                if model is None:
                    raise ValueError(f"stream {ev!r}: the history does not hold this event type and was built without a model to take its columns from")
                new_cols[ev] = self._col_map(self.sess, model, ev)
            elif (times is None) != (st.times is None):
                raise ValueError(f"stream {ev!r}: the stream {'has no times' if st.times is None else 'has times'}, the batch must agree")
        if n_users is None:
            n_users = len(user_ids) if user_ids is not None else max([int(u.max().item()) + 1 for u, _, _ in streams.values() if u.numel()] + [self.n_users])
        n_users = int(n_users)
        if n_users < self.n_users:
            raise ValueError(f"n_users {n_users} is below the history's {self.n_users}: the user id space does not shrink")
        for ev, st in self.types.items():      # a stream of unknown length (a _Stream built without n_events) cannot be appended to or extended
            if st.n_events < 0 and (n_users != self.n_users or (ev in streams and streams[ev][0].numel())):
                raise ValueError(f"stream {ev!r}: built without its number of events (_Stream.n_events)")
        sess = self.sess
        for ev in list(self.types) + [ev for ev in streams if ev not in self.types]:
            st = self.types.get(ev)
            users, items, times = streams.get(ev, (None, None, None))
            n_new = int(users.numel()) if users is not None else 0
            if st is None:
                n_cols, col_map = new_cols[ev]
                st = self.types[ev] = _Stream(n_cols, None, None, None, None, col_map, n_events=0)
                have_times = times is not None
            else:
                have_times = st.times is not None
                if n_new == 0 and n_users == self.n_users:
                    continue
            n_old = st.n_events
            n = n_old + n_new
            if n_new or st.items is None:
                st.items_buf = self._grown(st.items_buf, st.items, n_old, n, torch.int32)
                st.items_buf[n_old:n].copy_(items)
                st.items = st.items_buf[:n] if n else st.items_buf[:1]      # an empty stream still has an array
                if have_times:
                    st.times_buf = self._grown(st.times_buf, st.times, n_old, n, torch.int64)
                    st.times_buf[n_old:n].copy_(times)
                    st.times = st.times_buf[:n] if n else st.times_buf[:1]
            out = st.idx_spare
            if out is None or out[0].numel() < n_users + 1 or out[1].numel() < n:
                live = st.idx_buf if st.idx_buf is not None else (st.idx_row_ptr, st.idx_pos)
                caps = [t.numel() if t is not None else 0 for t in live]      # the size of the live pair where that suffices, GROWTH times it where not
                caps = [c if c >= need else max(need, GROWTH * c, 1) for c, need in zip(caps, (n_users + 1, n))]
                out = (sess.empty(caps[0], torch.int64), sess.empty(caps[1], torch.int32))
            rp, pos = sess.history_append(st.idx_row_ptr, st.idx_pos, n_old, users if users is not None else sess.empty(0, torch.int32), n_users, out)
            st.idx_spare = st.idx_buf if st.idx_buf is not None else ((st.idx_row_ptr, st.idx_pos) if st.idx_row_ptr is not None else None)
            st.idx_buf, st.idx_row_ptr, st.idx_pos, st.n_events = out, rp, pos if n else out[1][:1], n
        self.n_users = n_users
        if user_ids is not None:
            self.user_ids = user_ids
        return self

    def trim(self, before_ms: Optional[int] = None, drop_users=None, events: Optional[List[str]] = None, max_events_per_user=None) -> "DeviceHistory":
        """Retention, in place (decision D22 of DESIGN.md; include/urcco.h urcco_dev_history_trim); returns self.  before_ms: the events with time <
        before_ms leave the event types named in `events` (default: every type that has times) -- the reference's eventWindow.  drop_users: an
        iterable of user keys (resolved through user_indices, once per call; unknown ones ignored) or an int32 tensor of dense ids; their events leave EVERY event type,
        whatever `events` says -- the event store's $delete of a user.  The users keep their ids: user_ids and n_users are unchanged, a dropped user
        is answered like a user without events.  Every result afterwards is the one of from_streams over the filtered whole streams with the same
        n_users; `append` works on as before.

        max_events_per_user (decision D27; urcco_dev_history_cap): None -- no cap, the call and the cost of before; an int -- of every user only that
        many most recent events (by time, then stream position; by position alone in a stream without times) stay in every type named in `events`
        (default: every type, with or without times); a dict {event: int} names the capped types itself, whatever `events` says.  The cap is decided on the
        stream as it is, independently of the other two rules.  Two consequences.  Exclusion rows read EVERY event of a blacklist type, not a window of
        them: a cap on a blacklist type shortens the blacklist -- the dict form exists so that a caller can leave such types out.  And
        `matrices` / train_from_history see only what is stored: a capped history trains on the capped events.  Term rows with max_items <= the cap
        are unchanged by it.

        A type for which no rule applies costs no call.  One device-to-host read, of the counts of all types together.  The outputs of the
        call become the stream's buffers, with the capacity the old ones had: their tail is the spare capacity the next append fills.  The index
        pair of before becomes the spare pair.  `last_trim` = {event: (events before, events after)} of the types that were trimmed.

        ValueError -- nothing is modified: `events` or the cap's dict names a type the history does not hold, or, with before_ms, `events` one without
        times; a cap below 1 or above 2^31 - 1; drop_users is a tensor of another dtype; a _Stream built by hand without n_events."""
        named = list(self.types) if events is None else list(events)
        for ev in named:
            if ev not in self.types:
                raise ValueError(f"trim: the history holds no event type {ev!r}")
            if before_ms is not None and events is not None and self.types[ev].times is None:
                raise ValueError(f"trim: the stream {ev!r} has no times, before_ms cannot apply to it")
        by_time = {ev for ev in named if self.types[ev].times is not None} if before_ms is not None else set()
        caps: Dict[str, int] = {}
        if isinstance(max_events_per_user, dict):
            caps = {ev: int(c) for ev, c in max_events_per_user.items()}
        elif max_events_per_user is not None:
            caps = {ev: int(max_events_per_user) for ev in named}
        for ev, c in caps.items():
            if ev not in self.types:
                raise ValueError(f"trim: the history holds no event type {ev!r}")
            if c < 1 or c > (1 << 31) - 1:
                raise ValueError(f"trim: max_events_per_user must be in 1 .. 2^31 - 1, got {c} for {ev!r}")
        sess = self.sess
        drop = None
        if isinstance(drop_users, torch.Tensor):
            if drop_users.dtype != torch.int32:
                raise ValueError("trim: drop_users as a tensor holds int32 dense user ids")
            drop = drop_users.reshape(-1).to(sess.device) if drop_users.numel() else None
        elif drop_users is not None:
            ids = [i for i in self.user_indices(drop_users) if i >= 0]
            drop = torch.tensor(ids, dtype=torch.int32).to(sess.device) if ids else None
        todo = [ev for ev in self.types if ev in by_time or drop is not None or ev in caps]
        for ev in todo:
            if self.types[ev].n_events < 0:
                raise ValueError(f"stream {ev!r}: built without its number of events (_Stream.n_events)")
        calls = []
        for ev in todo:      # every call first, then the one read of the counts; the history changes only after both
            st = self.types[ev]
            n = st.n_events
            if n == 0:
                continue
            spare = st.idx_spare
            if spare is None or spare[0].numel() < self.n_users + 1 or spare[1].numel() < n:
                live = st.idx_buf if st.idx_buf is not None else (st.idx_row_ptr, st.idx_pos)
                spare = (sess.empty(max(live[0].numel(), self.n_users + 1), torch.int64), sess.empty(max(live[1].numel(), n), torch.int32))
            out = (sess.empty((st.items_buf if st.items_buf is not None else st.items).numel(), torch.int32),
                   sess.empty((st.times_buf if st.times_buf is not None else st.times).numel(), torch.int64) if st.times is not None else None, spare[0], spare[1])
            cut = before_ms if ev in by_time else None
            if ev in caps:
                calls.append((ev, out, sess.history_cap(n, st.items, st.times, st.idx_row_ptr, st.idx_pos, caps[ev], cut, drop, out)[4]))
            else:
                calls.append((ev, out, sess.history_trim(n, st.items, st.times, st.idx_row_ptr, st.idx_pos, cut, drop, out)[4]))
        counts = torch.stack([c for _, _, c in calls]).cpu().tolist() if calls else []
        self.last_trim = {ev: (0, 0) for ev in todo}
        for (ev, (o_items, o_times, o_rp, o_pos), _), (k, _) in zip(calls, counts):
            st = self.types[ev]
            self.last_trim[ev] = (st.n_events, int(k))
            st.idx_spare = st.idx_buf if st.idx_buf is not None else (st.idx_row_ptr, st.idx_pos)
            st.items_buf, st.items = o_items, o_items[: max(k, 1)]      # an empty stream still has an array
            if o_times is not None:
                st.times_buf, st.times = o_times, o_times[: max(k, 1)]
            st.idx_buf, st.idx_row_ptr, st.idx_pos, st.n_events = (o_rp, o_pos), o_rp[: self.n_users + 1], o_pos[: max(k, 1)], int(k)
        return self

    def matrices(self, events: List[str], after_ms: Optional[int] = None, before_ms: Optional[int] = None, min_events_per_user: int = 1):
        """The Preparator's output from the resident streams (decision D23 of DESIGN.md; include/urcco.h urcco_dev_history_users / _matrix): one user x
        column matrix per event type of `events`, rows sorted and duplicate-free, over the events with after_ms <= time < before_ms (None: open).
        events[0] is the primary: the users with at least min_events_per_user of ITS events in the window (whatever their items) are the rows, numbered in
        ascending user id; the other types keep those users' events only.  Returns (row_of int32 [n_users] on the device: a user's row or -1, n_rows,
        {event: DevCsr}): every matrix has n_rows rows and the stream's n_cols columns -- what device.cross_occurrence_device takes.  The history itself is
        not modified.  Two device-to-host reads: n_rows, then the nnz of all matrices together.

        ValueError: `events` is empty or names a type the history does not hold; a window and a stream without times; min_events_per_user < 1; a
        _Stream built by hand without n_events."""
        from .device import DevCsr
        events = list(events)
        if not events:
            raise ValueError("matrices: at least the primary event type is needed")
        if int(min_events_per_user) < 1:
            raise ValueError(f"matrices: min_events_per_user must be >= 1, got {min_events_per_user}")
        for ev in events:
            st = self.types.get(ev)
            if st is None:
                raise ValueError(f"matrices: the history holds no event type {ev!r}")
            if st.n_events < 0:
                raise ValueError(f"stream {ev!r}: built without its number of events (_Stream.n_events)")
            if st.times is None and (after_ms is not None or before_ms is not None):
                raise ValueError(f"matrices: the stream {ev!r} has no times, a window cannot apply to it")
        sess = self.sess
        p = self.types[events[0]]
        row_of, n_rows_dev = sess.history_users(p.n_events, p.times, p.idx_row_ptr, p.idx_pos, after_ms, before_ms, int(min_events_per_user))
        n_rows = int(n_rows_dev.item())      # the first read: it sizes every row_ptr
        calls = {}
        for ev in events:
            if ev not in calls:
                st = self.types[ev]
                calls[ev] = sess.history_matrix(st.n_events, st.items, st.times, st.idx_row_ptr, st.idx_pos, st.n_cols, row_of, n_rows, after_ms, before_ms)
        nnz = torch.cat([c[2] for c in calls.values()]).cpu().tolist()      # the second read
        return row_of, n_rows, {ev: DevCsr(n_rows, self.types[ev].n_cols, rp, ci, int(k)) for (ev, (rp, ci, _)), k in zip(calls.items(), nnz)}

    def ranks(self, rankings, now_ms: Optional[int] = None, model_event_names=None) -> Dict[str, torch.Tensor]:
        """The backfill rank fields from the resident streams (decision D24 of DESIGN.md; include/urcco.h urcco_dev_history_ranks): PopModel.calc per entry
        of `rankings`, over the events the history holds instead of an event list on the host.  rankings: the dict form of pop_model.getRanks, {name?, type?,
        eventNames?, duration_s?, end_ms?} per ranking.  Returns {field name: int64 device tensor [model.n_items]} in the order of `rankings`, _lib.RANK_NONE
        where the item has no rank; the values are the reference's doubles as integers.  The field name defaults by type (pop_model.nameByType).
        eventNames None: the primary, model_event_names[0] (default: the model's first correlator); an empty list: every stream the history holds; a
        name it does not hold contributes nothing.  end = end_ms, else now_ms, else the clock; start = end - duration_s * 1000 (default 3650 days).
        Every stream position counts, whoever its user is.  `userDefined` and unknown types give a field of RANK_NONE throughout (the reference returns an
        empty RDD).  One call per ranking, no synchronisation; the history is not modified.

        ValueError: the history has no model; the type is `random` (not served from the history); a stream without times (every ranking is a window);
        a _Stream built by hand without n_events."""
        from . import _lib
        from .pop_model import RankingFieldName, RankingType, nameByType
        model = self.model
        if model is None:
            raise ValueError("ranks: the history was built without a model to take the primary's item dictionary from")
        if now_ms is None:
            import time
            now_ms = int(time.time() * 1000)
        primary = list(model_event_names[:1]) if model_event_names is not None else [model.correlators[0].name]
        codes = {RankingType.Popular: _lib.RANK_POPULAR, RankingType.Trending: _lib.RANK_TRENDING, RankingType.Hot: _lib.RANK_HOT}
        out: Dict[str, torch.Tensor] = {}
        for r in rankings:
            rtype = r.get("type") or RankingType.Popular
            if rtype == RankingType.Random:
                raise ValueError("ranks: `random` ranks are not served from the history")
            field = r.get("name") or nameByType.get(rtype, RankingFieldName.UnknownRank)
            if rtype not in codes:
                out[field] = torch.full((model.n_items,), _lib.RANK_NONE, dtype=torch.int64).to(self.sess.device)
                continue
            names = r["eventNames"] if r.get("eventNames") is not None else primary
            streams = []
            for ev in (list(dict.fromkeys(names)) if names else list(self.types)):
                st = self.types.get(ev)
                if st is None:
                    continue
                if st.n_events < 0:
                    raise ValueError(f"stream {ev!r}: built without its number of events (_Stream.n_events)")
                if st.times is None:
                    raise ValueError(f"ranks: the stream {ev!r} has no times, a ranking window cannot apply to it")
                streams.append((st.n_events, st.items, st.times, st.col_map, st.n_cols))
            end = int(r["end_ms"] if r.get("end_ms") is not None else now_ms)
            start = end - int(r.get("duration_s", 3650 * 86400)) * 1000
            out[field] = self.sess.history_ranks(streams, model.n_items, codes[rtype], start, end)
        return out

    @staticmethod
    def from_dict(sess: DeviceSession, model, history: Dict[str, Dict[str, List[str]]]) -> "DeviceHistory":
        """The dict form of batch_predict's `history` (user -> {event name: [item ids, oldest first]}) loaded onto the device: every user gets a
        dense id, the list order is the time order, an item outside the event's column dictionary gets the id -1."""
        user_ids = {u: i for i, u in enumerate(history)}
        return DeviceHistory.from_streams(sess, model, DeviceHistory._dict_streams(sess, model, history, user_ids), user_ids)

    @staticmethod
    def _dict_streams(sess: DeviceSession, model, history: Dict[str, Dict[str, List[str]]], user_ids: Dict) -> Dict[str, Tuple[torch.Tensor, torch.Tensor, None]]:
        """The streams of the dict form: per event name the users' lists one after the other, each in its own order; no times"""
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
        return streams

    def append_dict(self, model, history: Dict[str, Dict[str, List[str]]]) -> "DeviceHistory":
        """`append` for the dict form of from_dict (user -> {event name: [item ids, oldest first]}): the lists are appended in order behind what the
        history holds of the user, a user it has not seen gets the next id.  Only for a history whose user_ids is a dict (from_dict's)."""
        if not isinstance(self.user_ids, dict):
            raise ValueError("append_dict needs a history whose user_ids is a dict (DeviceHistory.from_dict)")
        user_ids = dict(self.user_ids)
        for u in history:
            user_ids.setdefault(u, len(user_ids))
        return self.append(self._dict_streams(self.sess, model, history, user_ids), user_ids, model=model)
