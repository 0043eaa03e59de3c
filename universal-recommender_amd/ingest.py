"""Device-side Preparator: `Preparator.prepare` (reference src/main/scala/Preparator.scala:44-87 and the two
IndexedDatasetSpark builders at :102-158, :160-214) on the GPU, from event streams of 64-bit keys.

The host keeps the id strings; it hands the device one pair of key arrays (user key, item key) per event type -- a 64-bit
hash of each string, or integer ids -- and gets back, per event type, the binary user x item CSR matrix in HBM plus, for
every dictionary, the stream position of each id's first occurrence (which is all it needs to rebuild the
id -> string BiDictionary: dense ids follow first appearance, decision D8 of DESIGN.md).  Semantics mirrored exactly:
  * the primary event type defines the ONE user dictionary; with `minEventsPerUser` only users with at least that many
    RAW primary events (duplicates included, :129-132) are kept, and the primary is rebuilt restricted to them so
    that items only dropped users touched vanish from its column dictionary (:57-63);
  * secondary event types drop events of users that are not in the dictionary, which is never extended (:173-179);
  * column dictionaries are per event type, over the events that survive the user filter (:184-186);
  * duplicates collapse (`setQuick(col, 1.0)`, :146, :205); all matrices have nrow = size(userDictionary) (:157, :213).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from .device import DevCsr, DeviceSession, _ptr


class DevDictionary:
    """urcco_key_table + the first-occurrence positions of its ids (first_pos[id] = index into the stream it was built from).

    `extend` makes the dictionary growable (decision D26 of DESIGN.md): a table built with min_count = 1 -- `dictionary_build` over no keys gives the empty
    one -- takes batch after batch, and answers every lookup as one build over all of them would.  first_pos speaks of the build's stream alone: it
    becomes None with the first id an extend adds, and dictionary_verify / _verify_against, which index it, are then refused (BAD_ARG); an extended
    dictionary is checked through extend(check_keys=...)."""

    def __init__(self, sess: DeviceSession, handle: C.c_void_p, n_ids: int, first_pos: torch.Tensor):
        self._sess = sess
        self.handle = handle
        self.n_ids = int(n_ids)
        self.first_pos = first_pos[: self.n_ids]
        self.check_keys: Optional[torch.Tensor] = None   # extend(check_keys=...): int64 [>= n_ids] on the device, the check key of every id's first appearance

    def with_check_keys(self, check_keys: torch.Tensor) -> "DevDictionary":
        """Seeds the per-id check keys of a dictionary that dictionary_build made: check_keys = the second hashes of the stream it was built from, gathered
        at first_pos.  Returns self."""
        if self.first_pos is None:
            raise ValueError("the dictionary was extended already: its first positions are gone")
        self.check_keys = check_keys[self.first_pos].clone() if self.n_ids else self._sess.empty(1, torch.int64)
        return self

    def extend(self, keys: torch.Tensor, select: Optional[torch.Tensor] = None, check_keys: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """A batch against the live table (urcco_dev_dictionary_extend): keys the dictionary knows keep their ids, the others get the next ids in order of
        first appearance.  Returns (ids int32 [n]: the id of every position, -1 where select[p] < 0; new_pos int64 [ids added]: the batch position of each
        new id's first appearance -- with the batch's strings the caller extends its id -> string list).  n_ids grows; one synchronisation.
        UrccoError BAD_ARG with the dictionary unchanged: a selected position holds the reserved key ~0, the table was built with min_count > 1, too many ids.

        check_keys (the second hashes of the batch's strings): the dictionary keeps one check key per id on the device -- those of the new ids are gathered
        at new_pos and appended to a buffer that grows as the history's buffers do (history.GROWTH) -- and HashCollision is raised when a position's check
        key differs from its id's.  A dictionary that holds ids needs them for every id (with_check_keys after the build, check_keys in every extend:
        ValueError otherwise, before anything changes).  After a HashCollision the batch IS in the dictionary: its other new keys have their ids and
        check keys, n_ids has grown; the colliding string shares the id of the string it collided with and has no id of its own -- re-key with another
        seed, as after a collision in the build."""
        from .history import GROWTH
        sess, n = self._sess, int(keys.numel())
        if check_keys is not None and int(check_keys.numel()) != n:
            raise ValueError("extend: one check key per key expected")
        if self.n_ids and (check_keys is None) != (self.check_keys is None):
            raise ValueError("extend: the dictionary keeps check keys for every id or for none (with_check_keys after the build, check_keys in every extend)")
        ids, new_pos = sess.empty(max(n, 1), torch.int32), sess.empty(max(n, 1), torch.int64)
        n_ids = C.c_int64()
        sess._check(sess.lib.urcco_dev_dictionary_extend(sess.handle, self.handle, n, _ptr(keys), _ptr(select), _ptr(ids), _ptr(new_pos), C.byref(n_ids)))
        n_before, self.n_ids = self.n_ids, int(n_ids.value)
        ids, new_pos = ids[:n], new_pos[: self.n_ids - n_before]
        if self.n_ids > n_before:
            self.first_pos = None
        if check_keys is not None:
            buf = self.check_keys
            if buf is None or int(buf.numel()) < self.n_ids:
                buf = sess.empty(max(self.n_ids, GROWTH * (int(buf.numel()) if buf is not None else 0), 1), torch.int64)
                if n_before:
                    buf[:n_before].copy_(self.check_keys[:n_before])
            buf[n_before: self.n_ids] = check_keys[new_pos]
            self.check_keys = buf
            took_part = ids >= 0
            bad = int((check_keys[took_part] != buf[ids[took_part].long()]).sum().item())
            if bad:
                err = HashCollision(f"two ids share a 64-bit key ({bad} position(s) of the batch carry another check key than their id)")
                err.n_mismatch = bad      # what dictionary_verify counts for a build
                raise err
        return ids, new_pos

    def close(self):
        if self.handle:
            self._sess.lib.urcco_key_table_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dictionary_build(sess: DeviceSession, keys: torch.Tensor, select: Optional[torch.Tensor] = None, min_count: int = 1) -> DevDictionary:
    """keys: uint64 stream as an int64 tensor (bit pattern); select: int32[n], positions with a negative entry are ignored.
    The key ~0 (the int64 -1) is reserved: a selected position that holds it makes the build fail with BAD_ARG."""
    n = keys.numel()
    first_pos = sess.empty(max(n, 1), torch.int64)
    handle, n_ids = C.c_void_p(), C.c_int64()
    sess._check(sess.lib.urcco_dev_dictionary_build(sess.handle, n, _ptr(keys), _ptr(select), int(min_count), _ptr(first_pos), C.byref(handle),
                                                    C.byref(n_ids)))
    return DevDictionary(sess, handle, n_ids.value, first_pos)


def dictionary_lookup(sess: DeviceSession, d: DevDictionary, keys: torch.Tensor, select: Optional[torch.Tensor] = None) -> torch.Tensor:
    ids = sess.empty(max(keys.numel(), 1), torch.int32)
    sess._check(sess.lib.urcco_dev_dictionary_lookup(sess.handle, d.handle, keys.numel(), _ptr(keys), _ptr(select), _ptr(ids)))
    return ids[: keys.numel()]


class HashCollision(RuntimeError):
    """Two different id strings share a 64-bit key (detected through the second hash); re-key with another seed."""


def dictionary_verify(sess: DeviceSession, d: DevDictionary, keys: torch.Tensor, check_keys: torch.Tensor, select: Optional[torch.Tensor] = None) -> int:
    """Number of stream positions whose check key differs from the check key of their id's first occurrence (0 = no collision)."""
    bad = C.c_int64()
    sess._check(sess.lib.urcco_dev_dictionary_verify(sess.handle, d.handle, keys.numel(), _ptr(keys), _ptr(select), _ptr(check_keys),
                                                     _ptr(d.first_pos) if d.n_ids else _ptr(sess.empty(1, torch.int64)), C.byref(bad)))
    return int(bad.value)


def dictionary_verify_against(sess: DeviceSession, d: DevDictionary, keys: torch.Tensor, check_keys: torch.Tensor, dict_check_keys: torch.Tensor,
                              select: Optional[torch.Tensor] = None) -> int:
    """dictionary_verify for another stream looked up in `d`: its check keys against the check keys of the ids' first occurrences
    in the stream the dictionary was built from."""
    bad = C.c_int64()
    sess._check(sess.lib.urcco_dev_dictionary_verify_against(sess.handle, d.handle, keys.numel(), _ptr(keys), _ptr(select), _ptr(check_keys), _ptr(dict_check_keys),
                                                             _ptr(d.first_pos) if d.n_ids else _ptr(sess.empty(1, torch.int64)), C.byref(bad)))
    return int(bad.value)


def csr_from_pairs(sess: DeviceSession, rows: torch.Tensor, cols: torch.Tensor, n_rows: int, n_cols: int) -> DevCsr:
    n = rows.numel()
    out_rp = sess.empty(n_rows + 1, torch.int64)
    out_ci = sess.empty(max(n, 1), torch.int32)
    nnz = C.c_int64()
    sess._check(sess.lib.urcco_dev_csr_from_pairs(sess.handle, n, _ptr(rows), _ptr(cols), n_rows, _ptr(out_rp), _ptr(out_ci), C.byref(nnz)))
    return DevCsr(n_rows, n_cols, out_rp, out_ci, int(nnz.value))


@dataclass
class DevPreparedEvent:
    name: str
    matrix: DevCsr                 # nrow = size of the user dictionary, ncol = size of this event type's item dictionary
    item_first_pos: torch.Tensor   # int64[ncol]: index into THIS event type's stream of each item id's first (surviving) occurrence


@dataclass
class DevPreparedData:
    user_first_pos: torch.Tensor   # int64[n_users]: index into the PRIMARY stream of each user id's first occurrence
    events: List[DevPreparedEvent]


def prepare_device(sess: DeviceSession, actions: Sequence[Tuple[str, torch.Tensor, torch.Tensor]],
                   min_events_per_user: Optional[int] = None) -> DevPreparedData:
    """Preparator.prepare.  actions[d] = (event name, user keys, item keys[, user check keys, item check keys]) with the keys
    as int64 tensors (uint64 bit patterns) resident on the session's device; actions[0] is the primary event type.  With
    check keys (a second, independent hash of the same strings) every dictionary is verified: HashCollision if two
    different strings were merged into one id.
    The key ~0 is the dictionaries' "empty slot" value: integer ids must not be -1 (UrccoError BAD_ARG for a stream that holds it at a position
    that takes part); preparator.hash_keys remaps the value for hashed strings."""
    if not actions:
        raise ValueError("need at least the primary event type")
    pu = actions[0][1]
    users = dictionary_build(sess, pu, None, min_events_per_user if min_events_per_user is not None else 1)
    try:
        n_users = users.n_ids
        user_first = users.first_pos.clone()
        if len(actions[0]) >= 5 and dictionary_verify(sess, users, pu, actions[0][3]):
            raise HashCollision("two user ids share a 64-bit key")
        out: List[DevPreparedEvent] = []
        for act in actions:
            name, uk, ik = act[0], act[1], act[2]
            if uk.numel() != ik.numel():
                raise ValueError(f"event type {name}: user and item key streams differ in length")
            if act is not actions[0] and len(act) >= 5 and len(actions[0]) >= 5 and dictionary_verify_against(sess, users, uk, act[3], actions[0][3]):
                raise HashCollision(f"event type {name}: a user id shares its 64-bit key with a different user id of the primary event type")
            rows = dictionary_lookup(sess, users, uk)                      # -1: user not in the dictionary -> event dropped
            items = dictionary_build(sess, ik, rows, 1)                     # column ids over the surviving events only
            try:
                if len(act) >= 5 and dictionary_verify(sess, items, ik, act[4], rows):
                    raise HashCollision(f"event type {name}: two item ids share a 64-bit key")
                cols = dictionary_lookup(sess, items, ik, rows)
                m = csr_from_pairs(sess, rows, cols, n_users, items.n_ids)
                out.append(DevPreparedEvent(name, m, items.first_pos.clone()))
            finally:
                items.close()
        return DevPreparedData(user_first, out)
    finally:
        users.close()
