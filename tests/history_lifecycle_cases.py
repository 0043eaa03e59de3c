"""DeviceHistory over its life (universal-recommender_amd/history.py; decisions D17, D21 - D24 and D26 of DESIGN.md): fixed schedules of about a dozen
interleaved appends and trims, run on ONE object whose buffers grow, carry stale tails and swap their spare pairs, checked after every step against
a host model that keeps the whole truth in numpy.  Shared by tests/test_sim_history_lifecycle.py and tests/test_gpu_history_lifecycle.py.

The promise under test: after any sequence of calls every result is bit for bit the one of from_streams over the surviving whole streams.  HostHistory
holds those streams -- concatenate, boolean filter, grow n_users, add an event type -- and does not import the product's history module; the
comparing is done by the restatements the kernel-level case libraries already hold (history_ref.rows_ref, history_append_cases.row_ptr_ref,
history_matrix_cases.users_ref / matrix_ref, history_ranks_cases.counts_ref / ranks_ref) and, end to end, by batch_predict over the dict form.

Three event types: "purchase" (the model's primary, with times), "view" (a secondary of the model, with times; the tests hang a column map on its
stream, as a model with string dictionaries would, so the exclusion rows and the ranks go through one), "wish" (outside the model, without times:
it can only feed exclusions).  Times are T0 + k * TICK for few k, so ties are the rule, with a handful of negative ones.

Every step of a schedule carries tags, the reasons it is there.  assert_schedule replays the schedule on the host model alone, proves every tag
at its step (capacities by the buffer rule of DeviceHistory.append's docstring: a buffer that is too small is replaced by one of max(needed, 2 * its
capacity) entries; a trim keeps the capacity) and that the tags together are REQUIRED: a step that is taken out, or no longer reaches its path,
fails there, before the device is touched.

The simulator runs the schedules at the size the GPU runs them (a few seconds): there is one size."""
import math
import os
import re
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import history_append_cases as A
import history_matrix_cases as M
import history_ranks_cases as R
import history_ref as H
import history_trim_cases as T

put = A.put
I64_MIN = H.I64_MIN
T0, TICK = T.T0, 500
EVENTS = ("purchase", "view", "wish")
N_ITEMS, N_VIEW, N_MODEL_ROWS = 400, 250, 1000
ROW_CAPS = T.ROW_CAPS                      # below, at and above the planted counts
GROWTH = 2                                 # the buffer rule, restated from DeviceHistory.append's docstring


def _constant(header, name):
    text = open(os.path.join(A.ROOT, "universal-recommender_amd", "csrc", header)).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


HA_TILE, HA_LDS_USERS = A.kernel_constants()
HT_CHUNK = _constant("cco_history.h", "HT_CHUNK")
SR_LDS = _constant("cco_sorted_rows.h", "SR_LDS")      # raw entries of a user the matrix kernel sorts in LDS; beyond: the bitmap class


PLANTED = (SR_LDS + 4, HT_CHUNK + 1, HT_CHUNK - 1, 300, 65, 64, 63, 1, 0)      # events of the planted users of the primary; the first: beyond the LDS row limit


# ---- the host model -------------------------------------------------------------------------------------------------------------------------------
class HostHistory:
    """The surviving events per event type, in stream order: streams[ev] = (users int32, items int32, times int64 | None); n_users; keys (a keyed
    history): user key -> dense id in order of first appearance, the event types of a batch walked in the order its dict lists them."""

    def __init__(self, keyed=False):
        self.n_users = 0
        self.streams = {}
        self.keys = {} if keyed else None

    def dense(self, batch):
        """the batch with its users as dense ids; a keyed history numbers the keys it has not seen"""
        if self.keys is None:
            return batch
        return {ev: (np.array([self.keys.setdefault(k, len(self.keys)) for k in users], np.int32), items, times) for ev, (users, items, times) in batch.items()}

    def append(self, batch, n_users=None):
        for ev, (users, items, times) in self.dense(batch).items():
            if ev in self.streams:
                u, i, t = self.streams[ev]
                assert (t is None) == (times is None)
                self.streams[ev] = (np.concatenate([u, users]), np.concatenate([i, items]), np.concatenate([t, times]) if t is not None else None)
            else:
                self.streams[ev] = (users.astype(np.int32), items.astype(np.int32), times)
        if self.keys is not None:
            n_users = len(self.keys)
        elif n_users is None:
            n_users = max([self.n_users] + [int(u.max()) + 1 for u, _, _ in batch.values() if u.size])
        assert n_users >= self.n_users
        self.n_users = int(n_users)

    def ids(self, users):
        """dense ids of trim's drop_users, as the history resolves them: unknown ones ignored"""
        if self.keys is not None:
            return [self.keys[k] for k in users if k in self.keys]
        return [int(u) for u in users if isinstance(u, (int, np.integer)) and 0 <= int(u) < self.n_users]

    def trim(self, before_ms=None, drop=(), events=None):
        drop = np.array(self.ids(drop), np.int64)
        for ev, (u, i, t) in self.streams.items():
            keep = ~np.isin(u, drop)
            if before_ms is not None and t is not None and (events is None or ev in events):
                keep &= t >= before_ms
            self.streams[ev] = (u[keep], i[keep], t[keep] if t is not None else None)

    def counts(self, ev):
        u = self.streams[ev][0]
        return np.bincount(u[(u >= 0) & (u < self.n_users)], minlength=self.n_users)

    def n_events(self, ev):
        return int(self.streams[ev][0].size)

    def copy(self):
        c = HostHistory(self.keys is not None)
        c.n_users, c.streams, c.keys = self.n_users, dict(self.streams), dict(self.keys) if self.keys is not None else None
        return c


# ---- schedules ------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Step:
    name: str
    op: str                             # "create" | "append" | "trim"
    tags: tuple
    batch: Optional[dict] = None        # create / append: event -> (users: int32 ids, or a list of key strings; items int32; times int64 | None)
    n_users: Optional[int] = None       # append of a dense history: stated explicitly (None: the default, the largest id + 1)
    before_ms: Optional[int] = None     # trim
    drop: Optional[list] = None
    events: Optional[list] = None
    fill: Optional[str] = None          # append: this event type's batch fills its buffer's spare capacity exactly
    full: bool = False                  # the matrices and the ranks after this step are part of the trace two runs must agree on


@dataclass
class Schedule:
    keyed: bool
    steps: list
    planted: list                       # dense ids of the users with planted counts: every one is a query user
    n_users_max: int


def _times(rng, n, lo, hi, negative=0):
    t = T0 + TICK * rng.integers(lo, hi, n).astype(np.int64)
    if negative:
        t[rng.permutation(n)[:negative]] = np.array([-5, -T0, I64_MIN + 1], np.int64)[rng.integers(0, 3, min(negative, n))]
    return t


def _events(rng, users, n_cols, ticks=None, negative=0, shuffle=True):
    """a batch of one event type over `users` (shuffled): random columns, one in seven outside the dictionary"""
    users = np.asarray(users, np.int32)
    if shuffle:
        users = users[rng.permutation(users.size)]
    items = rng.integers(0, n_cols, users.size).astype(np.int32)
    items[rng.random(users.size) < 0.15] = -1
    return users, items, _times(rng, users.size, ticks[0], ticks[1], negative) if ticks is not None else None


def _named(batch, name):
    """the users of a batch as key strings"""
    return {ev: ([name(int(x)) for x in u], i, t) for ev, (u, i, t) in batch.items()}


def _empty(timed):
    return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64) if timed else None


def make_dense_schedule():
    """from_streams / append / trim over dense ids.  The primary's first stream is laid out by user id for the index copy of the first append: the
    planted users (the heaviest first: whole tiles inside one user), a filler up to a tile boundary, HA_TILE + 5 users of one event (a whole tile of
    them), HA_LDS_USERS + 5 users of none (the next tile spans them all), then users of 0 .. 40 events."""
    rng = np.random.default_rng(71)
    planted = PLANTED
    filler = -sum(planted) % HA_TILE or HA_TILE
    counts = list(planted) + [filler] + [1] * (HA_TILE + 5) + [0] * (HA_LDS_USERS + 5) + rng.integers(0, 41, 800).tolist()
    n0 = len(counts)
    h = HostHistory()
    steps = []

    def add(step):
        steps.append(step)
        apply_host(h, step)

    early, late, later = (0, 200), (100, 300), (200, 400)      # ticks: the first streams; what arrives after the first time trim; after the second
    p0 = np.concatenate([np.repeat(np.arange(n0, dtype=np.int32), counts), np.full(9, -1, np.int32)])
    v_counts = rng.integers(0, 4, n0)
    v_counts[[0, 3, 4, 5]] = (900, 64, 65, 70)
    add(Step("create", "create", ("create",), {"purchase": _events(rng, p0, N_ITEMS, early, negative=6), "view": _events(rng, np.repeat(np.arange(n0), v_counts), N_VIEW, early)},
             n_users=n0))
    # users of later batches: anybody but the first planted users, whose counts must still hold at the first trim
    some = lambda n, nobody=0: np.concatenate([rng.integers(len(planted) + 1, h.n_users, n), np.full(nobody, -1)])      # noqa: E731
    add(Step("append: 2x growth, a new type", "append", ("grow_2x", "new_type_later", "copy_shapes", "nobody", "times"),
             {"purchase": _events(rng, some(3000, 7), N_ITEMS, early, negative=5), "view": _events(rng, some(1500, 3), N_VIEW, early), "wish": _events(rng, some(500, 2), N_ITEMS)},
             full=True))
    n_wish = h.n_events("wish")
    add(Step("append: both index pairs", "append", ("both_pairs",), {"purchase": _events(rng, some(200), N_ITEMS, early), "wish": _events(rng, some(300), N_ITEMS)}))
    spare = GROWTH * n_wish - h.n_events("wish")      # the last append doubled the buffer of the first: this much is left
    add(Step("append: exact fill", "append", ("exact_fill",), {"wish": _events(rng, some(spare), N_ITEMS)}, fill="wish"))
    add(Step("append: one more event", "append", ("pos_plus_one",), {"wish": _events(rng, some(1), N_ITEMS)}))
    add(Step("append: one more user", "append", ("n_users_plus_one", "index_extended"), {"purchase": _events(rng, [n0], N_ITEMS, early)}, n_users=n0 + 1))
    cnt = h.counts("purchase")
    heaviest, u64 = int(np.argmax(cnt)), int(np.flatnonzero(cnt == 64)[0])
    add(Step("trim: users", "trim", ("trim_users",), drop=[heaviest, u64, h.n_users + 50, heaviest]))
    add(Step("trim: time", "trim", ("trim_time_half", "trims_back_to_back"), before_ms=T0 + TICK * 100, full=True))
    new = np.arange(h.n_users, h.n_users + len(planted), dtype=np.int32)      # the planted counts again, on new users
    add(Step("append: planted counts again", "append", ("replant", "n_users_grows"),
             {"purchase": _events(rng, np.concatenate([np.repeat(new, planted), some(600, 4)]), N_ITEMS, late, negative=3), "view": _events(rng, some(900), N_VIEW, late)},
             n_users=h.n_users + 260))
    add(Step("append: n_users alone", "append", ("only_n_users",), {"purchase": _empty(True), "view": _empty(True), "wish": _empty(False)}, n_users=h.n_users + 100))
    cnt = h.counts("purchase")
    add(Step("trim: both rules", "trim", ("trim_both",), before_ms=T0 + TICK * 150, drop=[int(np.argmax(cnt)), 7, int(new[3])]))
    add(Step("trim: one type, to nothing", "trim", ("trim_one_type", "trim_empties"), before_ms=T0 + TICK * 1000, events=["view"]))
    add(Step("append: into the emptied stream", "append", ("append_into_empty", "need_wins"),
             {"view": _events(rng, some(800, 2), N_VIEW, later), "wish": _events(rng, some(3600), N_ITEMS), "purchase": _events(rng, some(700, 2), N_ITEMS, later)}))
    quiet = int(np.flatnonzero(h.counts("purchase") + h.counts("view") + h.counts("wish") == 0)[0])
    add(Step("trim: nothing", "trim", ("trim_nothing",), before_ms=-(1 << 62), drop=[quiet, h.n_users + 3], full=True))
    return Schedule(False, steps, list(range(len(planted))) + new.tolist() + [n0], h.n_users)


def make_keyed_schedule():
    """from_key_streams / append_keys / trim over key strings "u<j>": user j's dense id is decided by the order in which the batches first name it"""
    rng = np.random.default_rng(73)
    planted = PLANTED
    name = "u{}".format
    h = HostHistory(keyed=True)
    steps = []

    def add(step):
        steps.append(step)
        apply_host(h, step)

    early, late = (0, 200), (100, 300)
    counts = list(planted) + rng.integers(0, 12, 400).tolist()
    first = np.repeat(np.arange(len(counts)), counts)
    add(Step("create", "create", ("create",), _named({"purchase": _events(rng, first, N_ITEMS, early, negative=4), "view": _events(rng, rng.integers(0, 300, 1500), N_VIEW, early)}, name)))

    def known(n):      # users the dictionary holds, but for the planted ones: their counts must still hold at the first trim
        pool = np.array([j for j in (int(k[1:]) for k in h.keys) if j >= len(planted)])
        return pool[rng.integers(0, pool.size, n)]

    n_seen = len(h.keys)
    add(Step("append: known users", "append", ("known_only", "new_type_later", "grow_2x"),
             _named({"purchase": _events(rng, known(2500), N_ITEMS, early), "wish": _events(rng, known(400), N_ITEMS)}, name), full=True))
    fresh = np.arange(1000, 1300)
    add(Step("append: new users, the view first", "append", ("new_only", "type_order"),
             _named({"view": _events(rng, np.repeat(fresh, 2), N_VIEW, early), "purchase": _events(rng, np.repeat(fresh[::-1], 3), N_ITEMS, early)}, name)))
    cnt = h.counts("purchase")
    heaviest, u64 = int(np.argmax(cnt)), int(np.flatnonzero(cnt == 64)[0])
    by_id = {i: k for k, i in h.keys.items()}
    add(Step("trim: users", "trim", ("trim_users",), drop=[by_id[heaviest], by_id[u64], "nobody", by_id[heaviest]]))
    add(Step("append: mixed, a dropped user returns", "append", ("mixed", "dropped_returns"),
             _named({"purchase": _events(rng, np.concatenate([known(1500), np.full(40, int(by_id[heaviest][1:])), np.arange(2000, 2100)]), N_ITEMS, late, negative=2),
                     "view": _events(rng, known(700), N_VIEW, late)}, name)))
    add(Step("trim: time", "trim", ("trim_time_half",), before_ms=T0 + TICK * 100, full=True))
    add(Step("trim: both rules", "trim", ("trim_both", "trims_back_to_back"), before_ms=T0 + TICK * 120, drop=[by_id[3], "u2050", "nobody at all"]))
    again = np.arange(4000, 4000 + len(planted))      # the planted counts again, on new users
    add(Step("append: after the trims, planted counts again", "append", ("append_after_trims", "replant"),
             _named({"purchase": _events(rng, np.concatenate([np.repeat(again, planted), known(2000)]), N_ITEMS, late), "view": _events(rng, known(300), N_VIEW, late), "wish": _events(rng, known(500), N_ITEMS)}, name),
             full=True))
    add(Step("trim: unknown users alone", "trim", ("trim_unknown_only",), drop=["nobody", "u-7"]))
    later = np.arange(3000, 3050)
    add(Step("append: new users, the untimed type first", "append", ("new_by_untimed",),
             _named({"wish": _events(rng, later, N_ITEMS), "purchase": _events(rng, np.concatenate([np.repeat(later[::-1], 4), known(300)]), N_ITEMS, late)}, name), full=True))
    assert n_seen < len(h.keys)
    return Schedule(True, steps, [h.keys[name(j)] for j in range(len(planted)) if name(j) in h.keys] + [h.keys[name(j)] for j in again if name(j) in h.keys] + [h.keys["u1000"], h.keys["u2099"]], h.n_users)


def apply_host(h: HostHistory, step: Step):
    if step.op == "trim":
        h.trim(step.before_ms, step.drop or (), step.events)
    else:
        h.append(step.batch, step.n_users)


REQUIRED_DENSE = {"create", "both_pairs", "pos_plus_one", "grow_2x", "new_type_later", "copy_shapes", "nobody", "times", "n_users_plus_one", "index_extended", "exact_fill", "trim_users", "trim_time_half",
                  "trims_back_to_back", "replant", "n_users_grows", "only_n_users", "trim_both", "trim_one_type", "trim_empties", "append_into_empty", "need_wins", "trim_nothing"}
REQUIRED_KEYED = {"create", "known_only", "new_type_later", "grow_2x", "new_only", "type_order", "trim_users", "mixed", "dropped_returns", "trim_time_half", "trim_both",
                  "trims_back_to_back", "append_after_trims", "replant", "trim_unknown_only", "new_by_untimed"}


def _tiles(rp):
    """(first user, last user) of every HA_TILE entries of an index"""
    cnt = np.diff(rp)
    owner = np.repeat(np.arange(cnt.size), cnt)
    n_e = int(rp[-1])
    return cnt, [(int(owner[a]), int(owner[min(a + HA_TILE, n_e) - 1])) for a in range(0, n_e, HA_TILE)]


def _has_planted(cnt):
    return all((cnt == c).any() for c in PLANTED) and ((cnt > 100) & (cnt < 1000)).any()


def assert_schedule(s: Schedule):
    """From the host model alone, before any device call: every tag holds at its step, every required tag is there, and the shapes cross the kernels'
    constants.  Raises AssertionError."""
    h = HostHistory(s.keyed)
    cap = {}                                                        # event -> entries of its items buffer, by the buffer rule
    done = set()
    dropped = set()                                                 # dense ids a trim has named
    first_trim = None
    planted_before = planted_after = False
    assert s.steps[0].op == "create" and all(st.op in ("append", "trim") for st in s.steps[1:]) and 8 <= len(s.steps) <= 14
    assert any(st.full and st.op == "trim" for st in s.steps) and sum(st.full for st in s.steps) >= 3      # matrices and ranks directly after a trim
    for k, st in enumerate(s.steps):
        before = h.copy()
        tags = set(st.tags)
        if st.op != "trim":
            known_before = set(h.keys) if s.keyed else None
            batch = h.copy().dense(st.batch)
            grow, need_wins, exact, new_type = False, False, False, False
            for ev, (u, i, t) in batch.items():
                n_old = before.n_events(ev) if ev in before.streams else 0
                need = n_old + u.size
                if ev not in cap:
                    new_type |= k > 0
                    cap[ev] = max(need, 1)
                elif cap[ev] < need:
                    grow |= need < GROWTH * cap[ev]
                    need_wins |= need > GROWTH * cap[ev]
                    cap[ev] = max(need, GROWTH * cap[ev])
                elif u.size:
                    exact |= need == cap[ev] and ev == st.fill
            apply_host(h, st)
            if "create" in tags:
                assert k == 0 and all(u.size > 0 for u, _, _ in batch.values()) and batch["purchase"][2] is not None and batch["view"][2] is not None
            assert ("grow_2x" not in tags or grow) and ("need_wins" not in tags or need_wins) and ("exact_fill" not in tags or exact), (st.name, cap)
            assert (st.fill is not None) == ("exact_fill" in tags)
            if "new_type_later" in tags:
                assert new_type and h.streams["wish"][2] is None
            if "copy_shapes" in tags:                               # what the index copy of this append reads: the primary's old index
                rp = A.row_ptr_ref(before.streams["purchase"][0], before.n_users)
                cnt, tiles = _tiles(rp)
                assert batch["purchase"][0].size > 0 and len(tiles) >= 8 and 20_000 <= rp[-1] <= 60_000
                assert any(lo == hi for lo, hi in tiles), "no tile inside one user"
                assert any(hi - lo + 1 == HA_TILE and (cnt[lo:hi + 1] == 1).all() for lo, hi in tiles), "no tile of one-event users"
                assert any(hi - lo + 1 > HA_LDS_USERS for lo, hi in tiles), "no tile over more users than the staging holds"
                assert 2 * HA_LDS_USERS <= before.n_users <= 3 * HA_LDS_USERS
            if "nobody" in tags:
                assert all((u == -1).any() and (i == -1).any() for u, i, _ in batch.values())
            if "times" in tags:
                t = np.concatenate([before.streams["purchase"][2], batch["purchase"][2]])
                assert (t < 0).any() and np.unique(t).size < t.size // 20 and (batch["purchase"][2] < 0).any()
            if "both_pairs" in tags:                                # the second append behind the creation: from here on a live and a spare index pair exist
                assert k == 2 and s.steps[1].op == "append" and h.n_users == s.steps[0].n_users and all(x.batch["purchase"][0].size for x in s.steps[1:3])
                assert h.n_events("purchase") <= GROWTH * s.steps[0].batch["purchase"][0].size
            if "n_users_plus_one" in tags:                          # the row starts of both pairs have n_users + 1 entries: one short of the new id space
                assert h.n_users == before.n_users + 1 == s.steps[0].n_users + 1 and "both_pairs" in done and batch["purchase"][0].size == 1 and first_trim is None
            if "pos_plus_one" in tags:                              # the positions of both pairs have exactly the events of before, one short; the row starts suffice
                assert "exact_fill" in s.steps[k - 1].tags and s.steps[k - 1].fill == "wish" and batch["wish"][0].size == 1 and h.n_users == before.n_users
            if "index_extended" in tags:
                assert h.n_users > before.n_users and any(ev not in batch for ev in before.streams) and any(u.size for u, _, _ in batch.values())
            if "only_n_users" in tags:
                assert h.n_users > before.n_users and set(batch) == set(before.streams) and not any(u.size for u, _, _ in batch.values())
            if "n_users_grows" in tags:
                assert h.n_users - s.steps[0].n_users >= 200
            if "replant" in tags:
                assert first_trim is not None and _has_planted(h.counts("purchase"))
            if "append_into_empty" in tags:
                assert "trim_empties" in s.steps[k - 1].tags and any(before.n_events(ev) == 0 and batch[ev][0].size > 0 for ev in batch if ev in before.streams)
            if "append_after_trims" in tags:
                assert s.steps[k - 1].op == "trim" and all(ev in batch for ev in before.streams)
            if s.keyed:
                users = [x for us, _, _ in st.batch.values() for x in us]
                was = [x in known_before for x in users]
                assert ("known_only" not in tags or all(was)) and ("new_only" not in tags or not any(was)) and ("mixed" not in tags or (any(was) and not all(was)))
                if "type_order" in tags:                            # a new user's id comes from the type the dict lists first
                    evs = list(st.batch)
                    assert evs[0] != "purchase" and len(evs) > 1 and set(st.batch[evs[0]][0]) == set(st.batch[evs[1]][0]) and st.batch[evs[0]][0][0] != st.batch[evs[1]][0][0]
                if "new_by_untimed" in tags:                        # ids handed out while walking a type without times
                    ev0 = next(iter(st.batch))
                    assert h.streams[ev0][2] is None and not any(x in known_before for x in st.batch[ev0][0]) and s.steps[k - 1].op == "trim"
                if "dropped_returns" in tags:
                    back = [h.keys[x] for x in users if x in known_before and h.keys[x] in dropped]
                    assert back and all(h.counts("purchase")[i] > 0 for i in back)
        else:
            first_trim = k if first_trim is None else first_trim
            if first_trim == k:
                planted_before = _has_planted(h.counts("purchase"))
            ids = before.ids(st.drop or ())
            apply_host(h, st)
            dropped |= set(ids)
            n_before = {ev: before.n_events(ev) for ev in before.streams}
            n_after = {ev: h.n_events(ev) for ev in h.streams}
            cnt = before.counts("purchase")
            if "trim_users" in tags:
                assert st.before_ms is None and int(np.argmax(cnt)) in ids and any(cnt[i] == 64 for i in ids) and len(ids) > len(set(ids)) and len(st.drop) > len(ids)
            if "trim_time_half" in tags:
                assert not st.drop and 0.3 < n_after["purchase"] / n_before["purchase"] < 0.7 and n_after["view"] < n_before["view"]
            if "trims_back_to_back" in tags:
                assert s.steps[k - 1].op == "trim" and all(n_after[ev] < n_before[ev] for ev in ("purchase", "view"))
            if "trim_both" in tags:
                by_time = before.streams["purchase"][2] >= st.before_ms
                by_user = ~np.isin(before.streams["purchase"][0], ids)
                assert st.before_ms is not None and ids and (by_time & ~by_user).any() and (~by_time & by_user).any() and n_after["purchase"] > 0
            if "trim_one_type" in tags:
                assert st.events is not None and len(st.events) == 1 and not st.drop
                assert all((n_after[ev] < n_before[ev]) == (ev in st.events) for ev in n_before) and (before.streams["purchase"][2] < st.before_ms).any()
            if "trim_empties" in tags:
                assert any(n_before[ev] > 0 and n_after[ev] == 0 for ev in n_before)
            if "trim_unknown_only" in tags:                         # nobody the history knows: no call, no change
                assert st.drop and not ids and st.before_ms is None and n_after == n_before
            if "trim_nothing" in tags:                              # both rules are stated and reach every type: the calls run and keep everything
                assert n_after == n_before and min(n_before.values()) > 0 and st.before_ms is not None and ids
        if first_trim is not None and st.op == "append":
            planted_after |= _has_planted(h.counts("purchase"))
        done |= tags
    assert done == (REQUIRED_KEYED if s.keyed else REQUIRED_DENSE), done ^ (REQUIRED_KEYED if s.keyed else REQUIRED_DENSE)
    assert planted_before and planted_after, "the planted counts do not hold before the first trim and again after the appends that follow it"
    assert h.n_users == s.n_users_max and set(h.streams) == set(EVENTS)
    assert max(PLANTED) > SR_LDS > HT_CHUNK and SR_LDS >= HA_TILE
    q = query_users(s)
    assert q.size <= 320 and set(s.planted) <= set(q.tolist()) and (q >= s.n_users_max).any() and (q == -1).any() and any(i in q for i in dropped)


# ---- the checks of one step -----------------------------------------------------------------------------------------------------------------------
def query_users(s: Schedule):
    """every planted user, a fixed random sample, nobody, ids beyond the id space; in a fixed random order"""
    rng = np.random.default_rng(79)
    q = np.concatenate([s.planted, rng.integers(0, s.n_users_max, 250), [-1, s.n_users_max, s.n_users_max + 5]]).astype(np.int32)
    return q[rng.permutation(q.size)]


def view_col_map():
    rng = np.random.default_rng(83)
    m = rng.integers(0, N_ITEMS, N_VIEW).astype(np.int32)
    m[rng.random(N_VIEW) < 0.3] = -1
    return m


def _np(t):
    return t.cpu().numpy()


def check_state(dh, h: HostHistory):
    """n_users, the types, and per type the stream and its index against the host model"""
    assert dh.n_users == h.n_users and set(dh.types) == set(h.streams)
    for ev, (users, items, times) in h.streams.items():
        st = dh.types[ev]
        n = users.size
        assert st.n_events == n and st.items.numel() == max(n, 1) == st.idx_pos.numel() and st.idx_row_ptr.numel() == h.n_users + 1, ev
        assert np.array_equal(_np(st.items)[:n], items), ev
        assert (st.times is None) == (times is None) and (times is None or (st.times.numel() == max(n, 1) and np.array_equal(_np(st.times)[:n], times))), ev
        rp = _np(st.idx_row_ptr)
        assert np.array_equal(rp, A.row_ptr_ref(users, h.n_users)), ev
        pos = _np(st.idx_pos)[: int(rp[-1])].astype(np.int64)       # every user's segment, sorted, is flatnonzero(users == u): the segments' users are the
        owner = np.repeat(np.arange(h.n_users), np.diff(rp))        # positions' users, and together they are every somebody's position once
        assert np.array_equal(np.sort(pos), np.flatnonzero((users >= 0) & (users < h.n_users))) and np.array_equal(users[pos], owner), ev


def rows_problem(sess, dh, h: HostHistory, q_users, col_map):
    """history_ref's problem and DeviceProblem over the host model's streams and the object's LIVE tensors"""
    rng = np.random.default_rng(89)
    lens = rng.integers(0, 4, q_users.size)
    extra_rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    extra_ci = np.concatenate([np.sort(rng.choice(N_ITEMS, n, replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    evs = [ev for ev in EVENTS if ev in h.streams]
    streams = [H.Stream(dh.types[ev].n_cols, *h.streams[ev], col_map if ev == "view" else None, True) for ev in evs]
    p = H.Problem(h.n_users, N_ITEMS, streams, q_users, extra_rp, extra_ci)
    return H.DeviceProblem.over(sess, p, [(t.n_cols, t.idx_row_ptr, t.idx_pos, t.items, t.times, t.col_map) for t in (dh.types[ev] for ev in evs)])


def check_rows(sess, dh, h, q_users, col_map, caps=ROW_CAPS):
    d = rows_problem(sess, dh, h, q_users, col_map)
    assert [s.n_cols for s in d.p.streams] == [{"purchase": N_ITEMS, "view": N_VIEW, "wish": N_ITEMS}[ev] for ev in EVENTS if ev in h.streams]
    out = []
    for cap in caps:
        _, terms, excl = H.check(d, [cap] * len(d.ev))
        out.append((terms, excl))
    return out


MATRIX_WINDOW = (T0 + TICK * 40, T0 + TICK * 240)


def rankings(h):
    """popular / trending / hot over windows that end behind the primary's latest event and begin at a tenth of its times: every interval holds events"""
    t = np.sort(h.streams["purchase"][2])
    end = int(t[-1]) + 1
    span = (end - int(t[t.size // 10])) // 1000 + 1
    return [{"name": "pop", "type": "popular", "eventNames": ["purchase", "view"], "duration_s": span, "end_ms": end},
            {"name": "trend", "type": "trending", "eventNames": ["purchase"], "duration_s": span, "end_ms": end + 7},
            {"name": "hot", "type": "hot", "eventNames": ["view", "purchase", "no such event"], "duration_s": span - 1, "end_ms": end}]


def _mat_problem(h, ev, n_cols, seed):
    users, items, times = h.streams[ev]
    return M.from_users(ev, users, h.n_users, n_cols, items, times, np.random.default_rng(seed))


def check_matrices(dh, h: HostHistory):
    """dh.matrices against users_ref / matrix_ref over an index built on the host: a window with min_events_per_user 2 over the timed types, and no
    window over all three.  Returns the device results as numpy."""
    out = []
    for events, window, min_events in ((["purchase", "view"], MATRIX_WINDOW, 2), (list(EVENTS), (None, None), 1)):
        events = [ev for ev in events if ev in h.streams]
        lo, hi = (M.I64_MIN if window[0] is None else window[0]), (M.I64_MAX if window[1] is None else window[1])
        row_of, n_rows, mats = dh.matrices(events, window[0], window[1], min_events)
        prim = _mat_problem(h, events[0], dh.types[events[0]].n_cols, 1)
        w_row_of, w_n_rows, c = M.users_ref(prim, lo, hi, min_events)
        assert n_rows == w_n_rows and np.array_equal(_np(row_of), w_row_of), (events, n_rows, w_n_rows)
        assert 0 < n_rows < h.n_users and (min_events == 1 or ((c > 0) & (c < min_events)).any())
        for k, ev in enumerate(events):
            t = _mat_problem(h, ev, dh.types[ev].n_cols, 2 + k)
            w_rp, w_ci = M.matrix_ref(t, lo, hi, w_row_of, w_n_rows, t.n_events)
            m = mats[ev]
            assert m.n_rows == n_rows and m.n_cols == t.n_cols and m.nnz_bound == w_ci.size, (ev, m.nnz_bound, w_ci.size)
            rp, ci = _np(m.row_ptr), _np(m.col_idx)[: w_ci.size]
            assert np.array_equal(rp, w_rp) and np.array_equal(ci, w_ci), ev
            out += [rp, ci]
        out.append(_np(row_of))
    return out


def check_ranks(dh, h: HostHistory, col_map):
    asked = rankings(h)
    got = dh.ranks(asked, now_ms=0)
    assert list(got) == [r["name"] for r in asked]
    codes = {"popular": R.POPULAR, "trending": R.TRENDING, "hot": R.HOT}
    out = []
    for r in asked:
        streams = [R.RStream(h.streams[ev][1], h.streams[ev][2], col_map if ev == "view" else None, dh.types[ev].n_cols) for ev in dict.fromkeys(r["eventNames"]) if ev in h.streams]
        end = r["end_ms"]
        want = R.ranks_ref(R.counts_ref(streams, N_ITEMS, codes[r["type"]], end - r["duration_s"] * 1000, end))
        rank = _np(got[r["name"]])
        assert np.array_equal(rank, want), (r["name"], rank[:20], want[:20])
        assert (want != R.NONE).any()
        out.append(rank)
    return out


def dict_form(h: HostHistory, who, name):
    """the dict batch_predict takes, user -> {event: [ids, oldest first]}, of the users `who`: equal times in stream order; an event outside the
    column dictionary (-1) carries an id no dictionary holds"""
    out = {name(u): {} for u in who}
    for ev, (users, items, times) in h.streams.items():
        beyond = max(N_ITEMS, N_VIEW) + 7
        for u in who:
            pos = np.flatnonzero(users == u)
            if times is not None:
                pos = pos[np.lexsort((pos, times[pos]))]
            out[name(u)][ev] = [int(i) if i >= 0 else beyond for i in items[pos]]
    return out


def check_predict(stack, dh, h: HostHistory, s: Schedule):
    """batch_predict over the object == over the dict form of the host model, with and without idf weights; "wish" and the primary blacklisted"""
    algo, model = stack
    by_id = {i: k for k, i in h.keys.items()} if s.keyed else None
    name = (lambda u: by_id[u]) if s.keyed else (lambda u: u)
    rng = np.random.default_rng(97)
    who = sorted({u for u in list(s.planted) + rng.integers(0, h.n_users, 40).tolist() if u < h.n_users})
    hist = dict_form(h, who, name)
    qs = [{"user": name(u)} for u in who] + [{"user": name(u), "item": int(u) % N_ITEMS} for u in who[::5]] + [{"user": name(u), "userBias": -1.0, "num": 5} for u in who[1::4]]
    qs += [{"user": name(u), "eventNames": ["view", "purchase", "wish"]} for u in who[2::3]]      # "wish" feeds exclusions only when a query names it
    qs += [{"user": "nobody" if s.keyed else s.n_users_max + 9}, {}, {"item": 5}]
    algo.ap.blacklistEvents = ["purchase", "wish"]
    try:
        for weights in (None, "idf"):
            want = algo.batch_predict(model, qs, hist, term_weights=weights)
            got = algo.batch_predict(model, qs, dh, term_weights=weights)
            for q, w, g in zip(qs, want, got):
                assert g == w, (weights, q, g, w)
            assert any(x["score"] > 0 for r in want for x in r["itemScores"])
    finally:
        algo.ap.blacklistEvents = None


# ---- the buffer contract, from the object alone ---------------------------------------------------------------------------------------------------
class Buffers:
    """Per event type: how often the buffer behind the items, the times and the index pair was replaced, and the capacities around every trim."""

    def __init__(self):
        self.first, self.last, self.ptr, self.changes, self.trims, self.fresh_pairs = {}, {}, {}, {}, {}, {}
        self.reused = 0                 # appends that merged into the spare pair

    @staticmethod
    def _bufs(st):
        pair = st.idx_buf if st.idx_buf is not None else (st.idx_row_ptr, st.idx_pos)
        return {"items": st.items_buf if st.items_buf is not None else st.items, "times": (st.times_buf if st.times_buf is not None else st.times), "rp": pair[0], "pos": pair[1]}

    def snapshot(self, dh):
        return {ev: (self._bufs(st), st.idx_spare, st.n_events) for ev, st in dh.types.items()}

    def after(self, dh, step: Step, was):
        for ev, st in dh.types.items():
            bufs = self._bufs(st)
            old = was.get(ev)
            trimmed = step.op == "trim" and old is not None and ev in dh.last_trim and old[2] > 0
            self.trims[ev] = self.trims.get(ev, 0) + trimmed
            for k, b in bufs.items():
                if b is None:
                    continue
                key = (ev, k)
                self.first.setdefault(key, b.numel())
                self.last[key] = b.numel()
                if key in self.ptr and self.ptr[key] != b.data_ptr() and k in ("items", "times"):
                    self.changes[key] = self.changes.get(key, 0) + 1
                self.ptr[key] = b.data_ptr()
            if old is not None:
                spare_ptrs = {t.data_ptr() for t in (old[1] or ())}
                if bufs["rp"].data_ptr() not in spare_ptrs | {old[0]["rp"].data_ptr()}:      # neither the live pair nor the spare pair of before: a new one
                    self.fresh_pairs[ev] = self.fresh_pairs.get(ev, 0) + 1
                    # its capacity: an append's has the live buffer's where that suffices and max(needed, GROWTH * it) where not (the rule of the stream
                    # buffers); a trim's has room for the index of before and no less than the live pair it replaces
                    for k, need in (("rp", dh.n_users + 1), ("pos", st.n_events if step.op == "append" else old[2])):
                        live = old[0][k].numel()
                        want = (live if live >= need else max(need, GROWTH * live)) if step.op == "append" else max(live, need)
                        assert bufs[k].numel() == want, (step.name, ev, k, bufs[k].numel(), live, need)
            if step.op == "append" and old is not None and bufs["rp"].data_ptr() != old[0]["rp"].data_ptr():
                # a merge: the pair of before is the spare pair now, and the merge wrote into the spare pair of before where that was large enough
                assert st.idx_spare is not None and st.idx_spare[0].data_ptr() == old[0]["rp"].data_ptr() and st.idx_spare[1].data_ptr() == old[0]["pos"].data_ptr(), (step.name, ev)
                if old[1] is not None and old[1][0].numel() >= dh.n_users + 1 and old[1][1].numel() >= st.n_events:
                    assert bufs["rp"].data_ptr() == old[1][0].data_ptr() and bufs["pos"].data_ptr() == old[1][1].data_ptr(), (step.name, ev)
                    self.reused += 1
            if trimmed:
                # the outputs of a trim have exactly the capacity of the buffers they replace; the index pair of before is the spare pair now, and the
                # new one is the spare pair of before where that had room for the whole index of before (a new pair: its capacity is asserted above)
                assert bufs["items"].numel() == old[0]["items"].numel() and (bufs["times"] is None or bufs["times"].numel() == old[0]["times"].numel()), (step.name, ev)
                assert st.idx_spare[0].data_ptr() == old[0]["rp"].data_ptr() and st.idx_spare[1].data_ptr() == old[0]["pos"].data_ptr(), (step.name, ev)
                assert bufs["rp"].numel() >= dh.n_users + 1 and bufs["pos"].numel() >= old[2], (step.name, ev)
                if old[1] is not None and old[1][0].numel() >= dh.n_users + 1 and old[1][1].numel() >= old[2]:
                    assert bufs["rp"].data_ptr() == old[1][0].data_ptr() and bufs["pos"].data_ptr() == old[1][1].data_ptr(), (step.name, ev)
                assert bufs["items"].data_ptr() != old[0]["items"].data_ptr() and bufs["rp"].data_ptr() != old[0]["rp"].data_ptr()
            elif step.op == "trim" and old is not None:             # a type the trim did not touch keeps its tensors
                assert all(b is None or b.data_ptr() == old[0][k].data_ptr() for k, b in bufs.items()), (step.name, ev)

    def check(self):
        """The items and the times buffer are replaced at most ceil(log2(final / first)) + 1 times, plus once per trim: every replacement by an append at
        least doubles them.  The index lives in a live and a spare pair that take turns, so its pointers change with every merge and a count of pointer
        changes says nothing; what is counted instead is the number of NEW pairs (neither the live nor the spare pair of before), against the same bound
        over the larger growth of its two buffers: pairs that did not grow geometrically fail it.  The capacity of every new pair is asserted where
        it appears (`after`)."""
        steps = lambda key: math.ceil(math.log2(self.last[key] / self.first[key])) + 1      # noqa: E731
        for (ev, k) in self.last:
            if k in ("items", "times"):
                assert self.changes.get((ev, k), 0) <= steps((ev, k)) + self.trims[ev], (ev, k, self.changes.get((ev, k), 0), self.first[ev, k], self.last[ev, k], self.trims[ev])
        assert self.reused > 0, "no append found its spare pair large enough"
        for ev, n in self.fresh_pairs.items():
            assert n <= max(steps((ev, "rp")), steps((ev, "pos"))) + self.trims[ev], (ev, n, steps((ev, "rp")), steps((ev, "pos")), self.trims[ev])
        return {"merges into the spare pair": self.reused, "changes": dict(self.changes), "new index pairs": dict(self.fresh_pairs), "trims": dict(self.trims), "first": dict(self.first), "last": dict(self.last)}


# ---- the run --------------------------------------------------------------------------------------------------------------------------------------
def stack_for(sess):
    """(algorithm, device model): history_ref.predict_stack over N_ITEMS items and N_VIEW view columns"""
    return H.predict_stack(sess, N_MODEL_ROWS, N_ITEMS, N_VIEW)


def _device_batch(sess, batch, keyed):
    from universal_recommender_amd.preparator import hash_keys
    out = {}
    for ev, (users, items, times) in batch.items():
        u = torch.from_numpy(hash_keys(list(users), library=sess.lib)).to(sess.device) if keyed else put(sess, np.asarray(users, np.int32))
        out[ev] = (u, put(sess, items), put(sess, times) if times is not None else None)
    return out


def run(sess, stack, s: Schedule, check=True):
    """The schedule on one object.  check: after EVERY step the state, the history rows, the matrices, the ranks and batch_predict against the host
    model, and at the end the buffer contract; without: the device calls alone (matrices and ranks on the steps marked `full`).  Returns the trace: per
    step what the device gave, as numpy arrays -- two runs must agree bit for bit (a user's index segment is a set, its order the hardware's: the
    trace holds the row starts only)."""
    from universal_recommender_amd.history import DeviceHistory
    assert_schedule(s)                                              # before the first device call
    algo, model = stack
    h = HostHistory(s.keyed)
    col_map = view_col_map()
    d_col_map = put(sess, col_map)
    q_users = query_users(s)
    buffers = Buffers()
    trace = []
    dh = None
    for step in s.steps:
        was = buffers.snapshot(dh) if dh is not None else {}
        if step.op == "create":
            batch = _device_batch(sess, step.batch, s.keyed)
            dh = DeviceHistory.from_key_streams(sess, model, batch) if s.keyed else DeviceHistory.from_streams(sess, model, batch, n_users=step.n_users)
        elif step.op == "append":
            if step.fill is not None:                               # the batch exactly fills what the object's buffer has left
                st = dh.types[step.fill]
                assert st.items_buf.numel() - st.n_events == len(step.batch[step.fill][0]) > 0, (st.items_buf.numel(), st.n_events)
            batch = _device_batch(sess, step.batch, s.keyed)
            assert (dh.append_keys(batch) if s.keyed else dh.append(batch, n_users=step.n_users)) is dh
            if step.fill is not None:
                assert st.items_buf.numel() == st.n_events and st.items_buf.data_ptr() == was[step.fill][0]["items"].data_ptr()
        else:
            n_before = {ev: st.n_events for ev, st in dh.types.items()}
            assert dh.trim(step.before_ms, step.drop, step.events) is dh
        apply_host(h, step)
        if "view" in dh.types and dh.types["view"].col_map is None:
            dh.types["view"].col_map = d_col_map
        if step.op == "trim":
            assert all(dh.last_trim[ev] == (n_before[ev], h.n_events(ev)) for ev in dh.last_trim), dh.last_trim
        buffers.after(dh, step, was)
        sess.synchronize()
        if check:
            check_state(dh, h)
            if s.keyed:
                asked = list(h.keys)[:: max(len(h.keys) // 50, 1)] + ["nobody", None, "u-1"]
                assert dh.user_indices(asked) == [h.keys.get(k, -1) if k is not None else -1 for k in asked] and dh.user_dict.n_ids == len(h.keys)
        rows = check_rows(sess, dh, h, q_users, col_map) if check else None
        if rows is None:
            d = rows_problem(sess, dh, h, q_users, col_map)
            terms, excl, _ = sess.history_rows(d.q_users, h.n_users, d.events([64] * len(d.ev)), N_ITEMS, d.extra)
            rows = [x for rp, ci in list(terms) + [excl] for x in (_np(rp), _np(ci)[: int(rp[-1])])]
        entry = [[_np(st.items)[: st.n_events] for st in dh.types.values()], [_np(st.times)[: st.n_events] for st in dh.types.values() if st.times is not None],
                 [_np(st.idx_row_ptr) for st in dh.types.values()], rows]
        if step.full or check:
            entry += [check_matrices(dh, h), check_ranks(dh, h, col_map)]
        if check:
            check_predict(stack, dh, h, s)
        trace.append(entry)
    if check:
        buffers.check()
    return trace


def same_trace(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return type(a) is type(b) and len(a) == len(b) and all(same_trace(x, y) for x, y in zip(a, b))
