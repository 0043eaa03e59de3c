"""Device-level driver of liburcco: the CCO model build with every matrix resident in HBM.

PyTorch is plumbing here (device memory, the HIP stream, torch.distributed for the RCCL exchange in
sharded.py); all arithmetic is the hand-written HIP behind include/urcco.h.  The stage order is the one Mahout's
SimilarityAnalysis.crossOccurrenceDownsampled runs on Spark (reference call sites URAlgorithm.scala:323-346):
column counts -> sampleDownAndBinarize -> column counts of the sample -> A.t -> per event type: A.t %*% B fused with
computeSimilarities (LLR + top-k).  Nothing in this path synchronises with the host.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch

from . import _lib


@dataclass
class DatasetParams:
    """Mahout DownsamplableCrossOccurrenceDataset limits, as URAlgorithm.scala:334-341 fills them."""
    max_elements_per_row: int = 500          # indicators[i].maxItemsPerUser / maxEventsPerEventType
    max_interesting_elements: int = 50       # indicators[i].maxCorrelatorsPerItem / maxCorrelatorsPerEventType
    min_llr: Optional[float] = None          # indicators[i].minLLR


@dataclass
class DevCsr:
    """Binary user x item matrix in HBM.  col_idx may be longer than the live nnz (capacity)."""
    n_rows: int
    n_cols: int
    row_ptr: torch.Tensor   # int64 [n_rows + 1]
    col_idx: torch.Tensor   # int32 [>= nnz]
    nnz_bound: int          # upper bound on nnz known to the host without a sync


@dataclass
class DevIndicators:
    """One indicator matrix (rows = items of A in [item_lo, item_hi), cols = items of B_i), CSR in HBM."""
    item_lo: int
    item_hi: int
    n_cols: int
    k: int
    row_ptr: torch.Tensor   # int64 [n + 1]
    col_idx: torch.Tensor   # int32 [n * k] (first row_ptr[-1] live)
    llr: torch.Tensor       # float64 [n * k]
    stats: torch.Tensor     # int64 [STATS_LEN]: pairs, then rows / pairs / users / emitted entries per accumulator bin; [STATS_LEN - 1]: rows of the
                            # micro class binned into its two shared-wave sub-lists (0: the build kept the class as one list)
    sampled_row_ptr: Optional[torch.Tensor] = None  # row_ptr of the down-sampled B this GPU multiplied with (several ranks: only the rows its
                                                    # item range touches are filled, include/urcco.h urcco_dev_result)
    sampled_col_idx: Optional[torch.Tensor] = None  # col_idx of the same (first sampled_row_ptr[-1] entries live)
    sampled_nnz_total: int = -1                     # entries of the WHOLE down-sampled matrix over all ranks (-1: one rank, = sampled_row_ptr[-1])

    def nnz_sampled_global(self) -> int:
        """nnz' of the whole matrix: the library's host-side total when the build exchanged, else the (whole) matrix this GPU holds."""
        if self.sampled_nnz_total >= 0:
            return int(self.sampled_nnz_total)
        return int(self.sampled_row_ptr[-1]) if self.sampled_row_ptr is not None and self.sampled_row_ptr.numel() else 0

    def to_host(self):
        if self.row_ptr.numel() == 0:
            import numpy as np
            return np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64)
        rp = self.row_ptr.cpu().numpy()
        nnz = int(rp[-1])
        return rp, self.col_idx[:nnz].cpu().numpy(), self.llr[:nnz].cpu().numpy()


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


class DeviceSession:
    """urcco_session bound to a torch device; launches go on torch's current stream for that device."""

    def __init__(self, device: torch.device, library=None, stream: Optional["torch.cuda.Stream"] = None):
        self.device = torch.device(device)
        self.lib = library if library is not None else _lib.lib()
        self.pack_counts = True   # cco_rows: B' with the columns' counts aboard (False: one count gather per candidate, the form of rounds 1-5)
        self.torch_stream = None
        handle = C.c_void_p()
        if self.device.type == "cuda":
            index = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self.device = torch.device("cuda", index)
            self.torch_stream = stream if stream is not None else torch.cuda.current_stream(self.device)
            self._check(self.lib.urcco_session_create(index, C.c_void_p(self.torch_stream.cuda_stream), C.byref(handle)))
        else:
            # only meaningful when the binding points at the test-only host-simulator build
            self._check(self.lib.urcco_session_create(0, None, C.byref(handle)))
        self.handle = handle

    def _check(self, status: int):
        _lib.check(status, self.lib)

    def close(self):
        if self.handle:
            self.lib.urcco_session_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._check(self.lib.urcco_session_synchronize(self.handle))

    def set_timing(self, enable: bool):
        self._check(self.lib.urcco_session_set_timing(self.handle, int(enable)))

    def set_debug(self, flags: int):
        self._check(self.lib.urcco_session_set_debug(self.handle, int(flags)))

    def expand_form(self) -> int:
        """0: the last cco_rows call of this session ran on narrow expand tables; else the reasons for the wide form (include/urcco.h); synchronises."""
        f = C.c_int32(-1)
        self._check(self.lib.urcco_session_expand_form(self.handle, C.byref(f)))
        return int(f.value)

    def set_expand_test(self, limit: int = 0, prefix_seed: int = 0):
        """Test hook: the scan-tile sum from which the expand tables take the wide form (0: the production value, 2^32), and where the work prefix starts."""
        self._check(self.lib.urcco_session_set_expand_test(self.handle, int(limit), int(prefix_seed)))

    def get_timings(self):
        """{stage name: (summed ms, launches)} since set_timing(True); synchronises."""
        ms = (C.c_double * _lib.N_STAGES)()
        n = (C.c_int64 * _lib.N_STAGES)()
        self._check(self.lib.urcco_session_get_timings(self.handle, ms, n))
        return {_lib.STAGE_NAMES[i]: (ms[i], n[i]) for i in range(_lib.N_STAGES) if _lib.STAGE_NAMES[i]}

    def empty(self, n, dtype):
        return torch.empty(int(n), dtype=dtype, device=self.device)

    # ---- stages ------------------------------------------------------------------------------------
    def column_counts(self, col_idx: torch.Tensor, nnz: int, n_cols: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        out = out if out is not None else self.empty(n_cols, torch.int32)
        self._check(self.lib.urcco_dev_column_counts(self.handle, nnz, _ptr(col_idx), n_cols, _ptr(out)))
        return out

    def downsample(self, m: DevCsr, nnz: int, raw_counts: torch.Tensor, seed: int, max_elements_per_row: int,
                   row_rate_mode: int = _lib.ROW_RATE_MAHOUT_INT_DIV, row_base: int = 0, post_out: Optional[torch.Tensor] = None):
        out_rp = self.empty(m.n_rows + 1, torch.int64)
        out_ci = self.empty(max(nnz, 1), torch.int32)
        post = post_out if post_out is not None else self.empty(max(m.n_cols, 1), torch.int32)
        self._check(self.lib.urcco_dev_downsample(self.handle, m.n_rows, _ptr(m.row_ptr), _ptr(m.col_idx), nnz, m.n_cols, _ptr(raw_counts),
                                                 _to_i32(seed), max_elements_per_row, row_rate_mode, row_base, _ptr(out_rp), _ptr(out_ci),
                                                 _ptr(post)))
        return DevCsr(m.n_rows, m.n_cols, out_rp, out_ci, nnz), post

    def transpose(self, m: DevCsr, counts: torch.Tensor, col_lo: int = 0, col_hi: Optional[int] = None):
        """CSC of m; only columns in [col_lo, col_hi) are materialised (the others are empty)."""
        col_hi = m.n_cols if col_hi is None else col_hi
        col_ptr = self.empty(m.n_cols + 1, torch.int64)
        row_idx = self.empty(max(m.nnz_bound, 1), torch.int32)
        self._check(self.lib.urcco_dev_transpose(self.handle, m.n_rows, _ptr(m.row_ptr), _ptr(m.col_idx), m.nnz_bound, m.n_cols, _ptr(counts),
                                                col_lo, col_hi, _ptr(col_ptr), _ptr(row_idx)))
        return col_ptr, row_idx

    def merge_fragments(self, world: int, item_lo: int, item_hi: int, n_items: int, lens: torch.Tensor, entries: torch.Tensor, n_entries: int,
                        sizes: torch.Tensor, counts: torch.Tensor):
        """CSC of the item range [item_lo, item_hi) from the fragments of `world` user shards (urcco_dev_merge_fragments):
        lens = uint16 or int32 column lengths, rank-major; entries = shard-local user ids, the fragments in rank order."""
        assert lens.dtype in (torch.uint16, torch.int16, torch.int32)
        col_ptr = self.empty(n_items + 1, torch.int64)
        row_idx = self.empty(max(n_entries, 1), torch.int32)
        self._check(self.lib.urcco_dev_merge_fragments(self.handle, world, item_lo, item_hi, n_items, _ptr(lens), int(lens.dtype != torch.int32), _ptr(entries),
                                                      n_entries, _ptr(sizes), _ptr(counts), _ptr(col_ptr), _ptr(row_idx)))
        return col_ptr, row_idx

    def row_work_csr(self, a: DevCsr, b_row_ptr: torch.Tensor) -> torch.Tensor:
        """Per-item work contributed by this user shard (sum over ranks = row_work)."""
        work = self.empty(max(a.n_cols, 1), torch.int64)
        self._check(self.lib.urcco_dev_row_work_csr(self.handle, a.n_rows, _ptr(a.row_ptr), _ptr(a.col_idx), a.nnz_bound, _ptr(b_row_ptr), a.n_cols,
                                                   _ptr(work)))
        return work[: a.n_cols]

    def row_work(self, item_lo: int, item_hi: int, n_items_a: int, a_col_ptr, a_row_idx, nnz_a_bound: int, b_row_ptr) -> torch.Tensor:
        work = self.empty(max(item_hi - item_lo, 1), torch.int64)
        self._check(self.lib.urcco_dev_row_work(self.handle, item_lo, item_hi, n_items_a, _ptr(a_col_ptr), _ptr(a_row_idx), nnz_a_bound,
                                                _ptr(b_row_ptr), _ptr(work)))
        return work[: item_hi - item_lo]

    def partition(self, work: torch.Tensor, n_parts: int) -> List[int]:
        bounds = (C.c_int32 * (n_parts + 1))()
        self._check(self.lib.urcco_dev_partition(self.handle, work.numel(), _ptr(work), n_parts, bounds))
        return list(bounds)

    def cco_rows(self, item_lo: int, item_hi: int, n_items_a: int, a_col_ptr, a_row_idx, nnz_a_bound: int, b: DevCsr, counts_a, counts_b,
                 n_users: int, exclude_self: bool, p: DatasetParams) -> DevIndicators:
        n = item_hi - item_lo
        k = p.max_interesting_elements
        o_count = self.empty(max(n, 1), torch.int32)
        o_idx = self.empty(max(n * k, 1), torch.int32)
        o_llr = self.empty(max(n * k, 1), torch.float64)
        stats = self.empty(_lib.STATS_LEN, torch.int64)
        # B' with the columns' counts aboard (round 6; what the context level does for every build): the row kernels read a candidate's cB off the
        # word that claims its accumulator slot.  pack_counts=False: the plain entry point with one count gather per candidate (rounds 1-5)
        if self.pack_counts and b.n_cols > 0:
            packed = self.empty(max(b.nnz_bound, 1), torch.int32)
            bad = self.empty(1, torch.int32)
            self._check(self.lib.urcco_dev_pack_counts(self.handle, b.n_rows, _ptr(b.row_ptr), _ptr(b.col_idx), b.nnz_bound, _ptr(counts_b), b.n_cols,
                                                      _ptr(packed), _ptr(bad)))
            self._check(self.lib.urcco_dev_cco_rows_packed(self.handle, item_lo, item_hi, n_items_a, _ptr(a_col_ptr), _ptr(a_row_idx), nnz_a_bound, _ptr(b.row_ptr),
                                                          _ptr(b.col_idx), b.n_cols, _ptr(counts_a), _ptr(counts_b), n_users, int(exclude_self), k,
                                                          int(p.min_llr is not None), float(p.min_llr) if p.min_llr is not None else 0.0,
                                                          _ptr(o_count), _ptr(o_idx), _ptr(o_llr), _ptr(stats), _ptr(packed), _ptr(bad)))
        else:
            self._check(self.lib.urcco_dev_cco_rows(self.handle, item_lo, item_hi, n_items_a, _ptr(a_col_ptr), _ptr(a_row_idx), nnz_a_bound, _ptr(b.row_ptr),
                                                   _ptr(b.col_idx), b.n_cols, _ptr(counts_a), _ptr(counts_b), n_users, int(exclude_self), k,
                                                   int(p.min_llr is not None), float(p.min_llr) if p.min_llr is not None else 0.0,
                                                   _ptr(o_count), _ptr(o_idx), _ptr(o_llr), _ptr(stats)))
        c_rp = self.empty(n + 1, torch.int64)
        c_idx = self.empty(max(n * k, 1), torch.int32)
        c_llr = self.empty(max(n * k, 1), torch.float64)
        self._check(self.lib.urcco_dev_compact_indicators(self.handle, n, k, _ptr(o_count), _ptr(o_idx), _ptr(o_llr), _ptr(c_rp), _ptr(c_idx),
                                                         _ptr(c_llr)))
        return DevIndicators(item_lo, item_hi, b.n_cols, k, c_rp, c_idx, c_llr, stats, b.row_ptr, b.col_idx)

    def recommend(self, n_queries: int, n_items: int, clauses, num: int, excl=None, item_mask: Optional[torch.Tensor] = None,
                  fill_order: Optional[torch.Tensor] = None, flags: int = 0, stats: bool = True, rules=None, weights=None):
        """urcco_dev_recommend: the top `num` of sum_c boost_c |T_c(q) ^ I_c(i)| per query row over the eligible items, in the order (score
        desc, backfill position asc).  clauses: (n_cols, boost, ind_col_ptr, ind_row_idx, q_row_ptr, q_col_idx) per should-clause, device
        tensors (the CSC of the indicator matrix, the CSR of the query terms); excl: (row_ptr, col_idx) of the exclusion CSR or None.
        Returns (count int32 [n_queries], idx int32 [n_queries, num], score float64 [n_queries, num], stats int64 [REC_STATS_LEN] or None);
        only the first count[q] entries of a row are written.  Enqueues, does not synchronise.
        rules (urcco_dev_recommend_rules; None = the rule-free call): per rule (RULE_ANY | RULE_NONE, n_cols, m_row_ptr, m_col_idx, q_row_ptr, q_col_idx)
        -- the CSR of the item x value matrix and of the query rows -- or (RULE_RANGE, item_value, q_lo, q_hi), int64 device tensors; an item is
        eligible only when every rule holds for (query, item).
        weights (urcco_dev_recommend_weighted, decision D20; None = the calls above): a list parallel to `clauses` of uint32 device tensors [n_cols] -- the
        clause's term weights in units of 2^-15, 1 .. REC_WEIGHT_MAX, e.g. from idf_weights -- or None for a clause whose terms all weigh REC_WEIGHT_ONE;
        the score is then sum_c boost_c * (sum of the weights of the shared terms) * 2^-15, still exact and independent of the order of the hits."""
        if weights is not None and len(weights) != len(clauses):
            raise ValueError("weights: one entry (a uint32 tensor or None) per clause")
        arr = (_lib.RecClause * max(len(clauses), 1))()
        for c, (n_cols, boost, cp, ri, qrp, qci) in enumerate(clauses):
            arr[c].n_cols, arr[c].boost = int(n_cols), float(boost)
            arr[c].ind_col_ptr, arr[c].ind_row_idx, arr[c].q_row_ptr, arr[c].q_col_idx = _ptr(cp), _ptr(ri), _ptr(qrp), _ptr(qci)
        o_count = self.empty(max(n_queries, 1), torch.int32)
        o_idx = self.empty(max(n_queries * num, 1), torch.int32)
        o_score = self.empty(max(n_queries * num, 1), torch.float64)
        st = self.empty(_lib.REC_STATS_LEN, torch.int64) if stats else None
        args = (self.handle, n_queries, n_items, arr, len(clauses), _ptr(excl[0]) if excl is not None else None, _ptr(excl[1]) if excl is not None else None,
                _ptr(item_mask), _ptr(fill_order), num, flags, _ptr(o_count), _ptr(o_idx), _ptr(o_score), _ptr(st))
        if rules is None and weights is None:
            self._check(self.lib.urcco_dev_recommend(*args))
        else:
            rules = rules or ()
            rl = (_lib.RecRule * max(len(rules), 1))()
            for j, rule in enumerate(rules):
                rl[j].kind = int(rule[0])
                if rule[0] == _lib.RULE_RANGE:
                    rl[j].item_value, rl[j].q_lo, rl[j].q_hi = (_ptr(t) for t in rule[1:4])
                else:
                    rl[j].n_cols = int(rule[1])
                    rl[j].m_row_ptr, rl[j].m_col_idx, rl[j].q_row_ptr, rl[j].q_col_idx = (_ptr(t) for t in rule[2:6])
            if weights is None:
                self._check(self.lib.urcco_dev_recommend_rules(*args, rl, len(rules)))
            else:
                for c, w in enumerate(weights):
                    if w is not None and (w.dtype != torch.uint32 or w.numel() < int(clauses[c][0])):
                        raise ValueError(f"weights[{c}]: a uint32 tensor of at least n_cols = {int(clauses[c][0])} entries")
                wp = (C.c_void_p * max(len(weights), 1))(*[_ptr(w) for w in weights])
                self._check(self.lib.urcco_dev_recommend_weighted(*args, rl, len(rules), wp))
        n = max(n_queries, 0)
        return o_count[:n], o_idx[: n * max(num, 0)].view(n, -1) if n and num > 0 else o_idx[:0], o_score[: n * max(num, 0)].view(n, -1) if n and num > 0 else o_score[:0], st

    def idf_weights(self, col_ptr: torch.Tensor, n_cols: int, n_docs: int) -> torch.Tensor:
        """urcco_dev_idf_weights: uint32 [n_cols], clamp(llrint(log(1 + (n_docs - df + 0.5) / (df + 0.5)) * 2^15), 1, REC_WEIGHT_MAX) with df the length of
        column h of the CSC whose column starts are col_ptr (int64 [n_cols + 1], device); a column nothing lists gets 1.  Enqueues, does not synchronise."""
        out = self.empty(max(n_cols, 1), torch.uint32)
        self._check(self.lib.urcco_dev_idf_weights(self.handle, n_cols, _ptr(col_ptr), n_docs, _ptr(out)))
        return out[: max(n_cols, 0)]

    def rank_metrics(self, count: torch.Tensor, idx: torch.Tensor, truth_row_ptr: torch.Tensor, truth_col_idx: torch.Tensor, ks, discount: Optional[torch.Tensor] = None,
                     sums: bool = True, out=None):
        """urcco_dev_rank_metrics (decision D19): hits, average precision and NDCG at the cut-offs `ks` of the recommendation table (count int32 [n], idx
        int32 [n, num], as recommend leaves them) against the truth rows (row_ptr int64 [n + 1], col_idx int32 sorted unique per row, e.g. a history term
        row).  ks: strictly ascending, each in 1..num.  discount: float64 [num] position weights of the DCG (None: no NDCG).
        Returns (hits int32 [n, n_ks], ap float64 [n, n_ks], ndcg float64 [n, n_ks] | None, sums_i int64 [2 + 2 n_ks] | None, sums_f float64 [2 n_ks] | None):
        sums_i = [evaluated, not evaluated, sum of hits per k, queries with a hit per k], sums_f = [tree sum of ap per k, of ndcg per k].
        out: (hits, ap, ndcg | None) contiguous tensors to write into instead of fresh ones.  Enqueues, does not synchronise."""
        n = int(count.numel())
        num = int(idx.shape[1]) if idx.dim() == 2 else (int(idx.numel()) // n if n else 1)
        ks = [int(k) for k in ks]
        ks_arr = (C.c_int32 * max(len(ks), 1))(*ks)
        if out is None:
            out = (self.empty(max(n * len(ks), 1), torch.int32), self.empty(max(n * len(ks), 1), torch.float64),
                   self.empty(max(n * len(ks), 1), torch.float64) if discount is not None else None)
        hits, ap, ndcg = (t.view(-1) if t is not None else None for t in out)
        s_i = self.empty(2 + 2 * len(ks), torch.int64) if sums else None
        s_f = self.empty(max(2 * len(ks), 1), torch.float64) if sums else None
        self._check(self.lib.urcco_dev_rank_metrics(self.handle, n, num, _ptr(count), _ptr(idx), _ptr(truth_row_ptr), _ptr(truth_col_idx), ks_arr, len(ks), _ptr(discount),
                                                   _ptr(hits), _ptr(ap), _ptr(ndcg), _ptr(s_i), _ptr(s_f)))
        shape = (n, len(ks))
        return (hits[: n * len(ks)].view(shape), ap[: n * len(ks)].view(shape), ndcg[: n * len(ks)].view(shape) if ndcg is not None else None, s_i,
                s_f[: 2 * len(ks)] if s_f is not None else None)

    def tree_sum(self, x: torch.Tensor) -> torch.Tensor:
        """urcco_dev_tree_sum: the pairwise sums of decision D19 over the rows of a contiguous float64 [n, n_cols] tensor, one per column: what
        `while x.size > 1: x = x[0::2] + x[1::2]` leaves of each column padded with +0.0 to a power of two.  Enqueues, does not synchronise."""
        n, n_cols = int(x.shape[0]), int(x.shape[1])
        out = self.empty(n_cols, torch.float64)
        self._check(self.lib.urcco_dev_tree_sum(self.handle, n, n_cols, _ptr(x), _ptr(out)))
        return out

    def history_index(self, users: torch.Tensor, n_users: int):
        """urcco_dev_history_index: the stream positions of every user's events.  users: int32 dense user id per event (< 0: nobody's).
        Returns (row_ptr int64 [n_users + 1], pos int32 [n_events]); the order inside a user's segment is unspecified.  Does not synchronise."""
        n = int(users.numel())
        row_ptr = self.empty(n_users + 1, torch.int64)
        pos = self.empty(max(n, 1), torch.int32)
        self._check(self.lib.urcco_dev_history_index(self.handle, n, _ptr(users), n_users, _ptr(row_ptr), _ptr(pos)))
        return row_ptr, pos

    def history_append(self, old_row_ptr: Optional[torch.Tensor], old_pos: Optional[torch.Tensor], n_old: int, new_users: torch.Tensor, n_users: int, out=None):
        """urcco_dev_history_append: the index of a stream that grew by the events of `new_users` (int32 dense user id of the stream positions n_old,
        n_old + 1, ...), from its old index (old_row_ptr int64 [n_users_old + 1], old_pos; both None: no old index) without the old stream's user ids.
        n_users >= n_users_old.  Returns (row_ptr int64 [n_users + 1], pos int32 [n_old + n_new]): per user the old segment as it was, then the new
        positions in unspecified order.  out: (row_ptr, pos) tensors of at least those sizes to write into -- they must not share memory with the old
        index; the returned tensors are views of them.  Does not synchronise."""
        n_old, n_new, n_users = int(n_old), int(new_users.numel()), int(n_users)
        n_users_old = int(old_row_ptr.numel()) - 1 if old_row_ptr is not None else 0
        row_ptr, pos = out if out is not None else (self.empty(n_users + 1, torch.int64), self.empty(max(n_old + n_new, 1), torch.int32))
        if row_ptr.numel() < n_users + 1 or pos.numel() < n_old + n_new:
            raise ValueError("history_append: the output tensors are smaller than n_users + 1 / n_old + n_new")
        self._check(self.lib.urcco_dev_history_append(self.handle, n_old, n_users_old, _ptr(old_row_ptr), _ptr(old_pos), n_new, _ptr(new_users), n_users,
                                                      _ptr(row_ptr), _ptr(pos)))
        return (row_ptr, pos) if out is None else (row_ptr[: n_users + 1], pos[: n_old + n_new])

    def history_trim(self, n_events: int, items: torch.Tensor, times: Optional[torch.Tensor], idx_row_ptr: torch.Tensor, idx_pos: torch.Tensor,
                     min_time_ms: Optional[int] = None, drop_users: Optional[torch.Tensor] = None, out=None):
        """urcco_dev_history_trim (decision D22): the stream (items int32, times int64 | None, n_events of them) and its index (idx_row_ptr int64
        [n_users + 1], idx_pos) without the events with time < min_time_ms (None: no time rule) and without the events of the users in drop_users
        (int32 dense ids in any order, repeats allowed, ids outside the id space ignored; None: nobody).  Returns (items, times | None, row_ptr, pos,
        counts): tensors sized by n_events (row_ptr: n_users + 1) of which the first K (items, times) and KE (pos) entries are the result, and counts
        int64 [2] = [K, KE] on the device.  out: (items, times | None, row_ptr, pos) tensors of at least those sizes to write into, returned as they
        are; they must not share memory with the inputs.  Does not synchronise."""
        n, n_users = int(n_events), int(idx_row_ptr.numel()) - 1
        n_drop = int(drop_users.numel()) if drop_users is not None else 0
        if out is None:
            out = (self.empty(max(n, 1), torch.int32), self.empty(max(n, 1), torch.int64) if times is not None else None, self.empty(n_users + 1, torch.int64),
                   self.empty(max(n, 1), torch.int32))
        o_items, o_times, o_rp, o_pos = out
        if o_items.numel() < n or o_pos.numel() < n or o_rp.numel() < n_users + 1 or (o_times is not None and o_times.numel() < n):
            raise ValueError("history_trim: the output tensors are smaller than n_events / n_users + 1")
        counts = self.empty(2, torch.int64)
        self._check(self.lib.urcco_dev_history_trim(self.handle, n, _ptr(items), _ptr(times), n_users, _ptr(idx_row_ptr), _ptr(idx_pos),
                                                    int(min_time_ms) if min_time_ms is not None and times is not None else -(1 << 63), n_drop,
                                                    _ptr(drop_users) if n_drop else None, _ptr(o_items), _ptr(o_times), _ptr(o_rp), _ptr(o_pos), _ptr(counts)))
        return o_items, o_times, o_rp, o_pos, counts

    def history_cap(self, n_events: int, items: torch.Tensor, times: Optional[torch.Tensor], idx_row_ptr: torch.Tensor, idx_pos: torch.Tensor,
                    max_per_user: Optional[int], min_time_ms: Optional[int] = None, drop_users: Optional[torch.Tensor] = None, out=None):
        """urcco_dev_history_cap (decision D27): history_trim with one more rule -- of every user only the max_per_user most recent events stay, by
        the rows' recency key (time, stream position); None: no cap, the outputs are history_trim's.  The three rules are independent and decided on
        the stream as passed in.  Arguments, result and `out` as in history_trim.  Does not synchronise."""
        n, n_users = int(n_events), int(idx_row_ptr.numel()) - 1
        n_drop = int(drop_users.numel()) if drop_users is not None else 0
        if out is None:
            out = (self.empty(max(n, 1), torch.int32), self.empty(max(n, 1), torch.int64) if times is not None else None, self.empty(n_users + 1, torch.int64),
                   self.empty(max(n, 1), torch.int32))
        o_items, o_times, o_rp, o_pos = out
        if o_items.numel() < n or o_pos.numel() < n or o_rp.numel() < n_users + 1 or (o_times is not None and o_times.numel() < n):
            raise ValueError("history_cap: the output tensors are smaller than n_events / n_users + 1")
        cap = (1 << 31) - 1 if max_per_user is None else int(max_per_user)
        if cap < 1 or cap > (1 << 31) - 1:
            raise ValueError(f"history_cap: max_per_user must be in 1 .. 2^31 - 1, got {max_per_user}")
        counts = self.empty(2, torch.int64)
        self._check(self.lib.urcco_dev_history_cap(self.handle, n, _ptr(items), _ptr(times), n_users, _ptr(idx_row_ptr), _ptr(idx_pos),
                                                   int(min_time_ms) if min_time_ms is not None and times is not None else -(1 << 63), n_drop,
                                                   _ptr(drop_users) if n_drop else None, cap, _ptr(o_items), _ptr(o_times), _ptr(o_rp), _ptr(o_pos), _ptr(counts)))
        return o_items, o_times, o_rp, o_pos, counts

    @staticmethod
    def _window(after_ms: Optional[int], before_ms: Optional[int]):
        return (-(1 << 63) if after_ms is None else int(after_ms), (1 << 63) - 1 if before_ms is None else int(before_ms))

    def history_users(self, n_events: int, times: Optional[torch.Tensor], idx_row_ptr: torch.Tensor, idx_pos: torch.Tensor, after_ms: Optional[int] = None,
                      before_ms: Optional[int] = None, min_events: int = 1):
        """urcco_dev_history_users (decision D23): which users of a stream's index train.  A user counts its index entries whose event lies in the window
        after_ms <= time < before_ms (None: open; a window needs `times`), whatever item the event carries.  Returns (row_of int32 [n_users]: the number of
        kept users below u when u has at least min_events such events, else -1; n_rows int64 [1] on the device).  Does not synchronise."""
        n_users = int(idx_row_ptr.numel()) - 1
        row_of = self.empty(max(n_users, 1), torch.int32)
        n_rows = self.empty(1, torch.int64)
        t_lo, t_hi = self._window(after_ms, before_ms)
        self._check(self.lib.urcco_dev_history_users(self.handle, int(n_events), _ptr(times), n_users, _ptr(idx_row_ptr), _ptr(idx_pos), t_lo, t_hi, int(min_events),
                                                     _ptr(row_of), _ptr(n_rows)))
        return row_of[:n_users], n_rows

    def history_matrix(self, n_events: int, items: torch.Tensor, times: Optional[torch.Tensor], idx_row_ptr: torch.Tensor, idx_pos: torch.Tensor, n_cols: int,
                       row_of: Optional[torch.Tensor] = None, n_rows: Optional[int] = None, after_ms: Optional[int] = None, before_ms: Optional[int] = None,
                       capacity: Optional[int] = None):
        """urcco_dev_history_matrix (decision D23): the user x column matrix of one event type from its stream (items int32, times int64 | None) and its
        index: row row_of[u] (None: u itself, n_rows = n_users) holds the distinct items of u's events in the window, ascending, those outside
        0 .. n_cols dropped.  Returns (row_ptr int64 [n_rows + 1], col_idx int32 [capacity], nnz int64 [1] on the device); capacity defaults to n_events,
        with which no row is lost.  Does not synchronise."""
        n, n_users = int(n_events), int(idx_row_ptr.numel()) - 1
        n_rows = n_users if n_rows is None else int(n_rows)
        capacity = n if capacity is None else int(capacity)
        row_ptr = self.empty(n_rows + 1, torch.int64)
        col_idx = self.empty(max(capacity, 1), torch.int32)
        nnz = self.empty(1, torch.int64)
        t_lo, t_hi = self._window(after_ms, before_ms)
        self._check(self.lib.urcco_dev_history_matrix(self.handle, n, _ptr(items), _ptr(times), n_users, _ptr(idx_row_ptr), _ptr(idx_pos), t_lo, t_hi, int(n_cols),
                                                      _ptr(row_of), n_rows, _ptr(row_ptr), _ptr(col_idx), capacity, _ptr(nnz)))
        return row_ptr, col_idx, nnz

    def history_ranks(self, streams, n_items: int, type: int, t_start: int, t_end: int, counts: bool = False):
        """urcco_dev_history_ranks (decision D24): the popular (1) / trending (2) / hot (3) rank of every item of the primary's dictionary from event streams
        on the device.  streams: per stream (n_events, items int32, times_ms int64 | None, col_map int32 | None, n_cols).  The window [t_start, t_end) is cut
        into `type` intervals; t_end = 2^63 - 1: no end.  Returns rank int64 [n_items] (_lib.RANK_NONE: no rank), with counts=True (rank, counts int32
        [type, n_items]).  Does not synchronise."""
        arr = (_lib.RankStream * max(len(streams), 1))()
        for k, (n, items, times, col_map, n_cols) in enumerate(streams):
            arr[k] = _lib.RankStream(int(n), _ptr(items), _ptr(times), _ptr(col_map), int(n_cols), 0)
        rank = self.empty(max(n_items, 1), torch.int64)
        cnt = self.empty(max(n_items * int(type), 1), torch.int32) if counts else None
        self._check(self.lib.urcco_dev_history_ranks(self.handle, arr, len(streams), int(n_items), int(type), int(t_start), int(t_end), _ptr(rank), _ptr(cnt)))
        rank = rank[:n_items]
        return (rank, cnt[: n_items * int(type)].view(int(type), n_items)) if counts else rank

    def fill_order(self, ranks) -> torch.Tensor:
        """urcco_dev_fill_order (decision D24): the backfill order of a model from up to _lib.RANK_MAX_FIELDS rank fields -- int64 device tensors of one length,
        _lib.RANK_NONE where an item has no rank: the items sorted by (field 0 desc, field 1 desc, ..., item id asc), an item without a rank last in its
        field.  Returns int32 [n_items].  Does not synchronise."""
        ranks = list(ranks)
        if not ranks:
            raise ValueError("fill_order: at least one rank field (a model without ranks has no fill order)")
        n_items = int(ranks[0].numel())
        if any(r.dtype != torch.int64 or int(r.numel()) != n_items for r in ranks):
            raise ValueError("fill_order: int64 rank fields of one length expected")
        if n_items == 0:
            return self.empty(0, torch.int32)
        ptrs = (C.c_void_p * len(ranks))(*[r.data_ptr() for r in ranks])
        out = self.empty(max(n_items, 1), torch.int32)
        self._check(self.lib.urcco_dev_fill_order(self.handle, n_items, ptrs, len(ranks), _ptr(out)))
        return out[:n_items]

    def history_rows(self, q_users: torch.Tensor, n_users: int, events, n_items: int, extra=None, stats: bool = False, timing: bool = False, keep_bounds: bool = False):
        """urcco_dev_history_bounds + urcco_dev_history_rows: the user-history term rows and the exclusion rows of a batch of queries.
        q_users: int32 [n_queries] dense user ids (< 0 or >= n_users: unknown).  events: per event type (n_cols, max_items, blacklist, idx_row_ptr, idx_pos,
        items, times_ms | None, col_map | None), device tensors (idx_*: history_index of the stream).  extra: (row_ptr, col_idx) of the caller's own
        exclusions per query, or None.  Returns (terms, excl, info): terms[t] = (row_ptr int64 [n_queries + 1], col_idx int32) sorted unique columns
        of the most recent max_items events, excl = the same pair over the primary's items, info = {"bounds": [...], "stats": int64 tensor | None,
        "ms": device time of the two calls | None, "bound_row_ptr": copies of the bounds' row_ptr arrays with keep_bounds (tests)}.  Reads the 1 + n_types bound totals between the two calls: one synchronisation."""
        nq = int(q_users.numel())
        arr = (_lib.HistEvent * max(len(events), 1))()
        rps = [self.empty(nq + 1, torch.int64) for _ in range(len(events) + 1)]   # the last: the exclusion rows
        for t, (n_cols, max_items, blacklist, irp, ipos, items, times, cmap) in enumerate(events):
            arr[t].n_cols, arr[t].max_items, arr[t].blacklist = int(n_cols), int(max_items), int(bool(blacklist))
            arr[t].idx_row_ptr, arr[t].idx_pos, arr[t].items, arr[t].times_ms, arr[t].col_map = _ptr(irp), _ptr(ipos), _ptr(items), _ptr(times), _ptr(cmap)
            arr[t].term_row_ptr = _ptr(rps[t])
        x_rp, x_ci = (_ptr(extra[0]), _ptr(extra[1])) if extra is not None else (None, None)
        head = (self.handle, nq, _ptr(q_users), n_users, arr, len(events), x_rp, x_ci)
        cis, info = self._bounded_rows(arr, len(events), nq, rps, stats, timing, keep_bounds,
                                       lambda: self.lib.urcco_dev_history_bounds(*head, _ptr(rps[-1])),
                                       lambda cis, totals, st: self.lib.urcco_dev_history_rows(*head, int(n_items), _ptr(rps[-1]), _ptr(cis[-1]), int(totals[-1]), _ptr(st)))
        return list(zip(rps[:-1], cis[:-1])), (rps[-1], cis[-1]), info

    def item_rows(self, q_items: torch.Tensor, specs, stats: bool = False, timing: bool = False, n_items: Optional[int] = None, keep_bounds: bool = False):
        """urcco_dev_item_bounds + urcco_dev_item_rows: the term rows of a batch of item queries, cut from the indicator matrices on the device.
        q_items: int32 [n_queries] dense item ids (< 0 or >= n_items: unknown, empty rows).  specs: per event type (n_cols, max_terms, ind_row_ptr,
        ind_col_idx), device tensors: the indicator CSR as the build left it, one row per item.  n_items: the rows of the matrices (default: from the
        first row_ptr).  Returns (rows, info): rows[t] = (row_ptr int64 [n_queries + 1], col_idx int32), the sorted distinct columns of the first
        max_terms entries of the item's row (max_terms - 1 when the row is longer); info = {"bounds": [...], "stats": int64 tensor | None, "ms":
        device time of the two calls | None, "bound_row_ptr": copies of the bounds' row_ptr arrays with keep_bounds (tests)}.  Reads the n_types bound
        totals between the two calls: one synchronisation."""
        nq = int(q_items.numel())
        if n_items is None:
            n_items = int(specs[0][2].numel()) - 1
        arr = (_lib.ItemEvent * max(len(specs), 1))()
        rps = [self.empty(nq + 1, torch.int64) for _ in specs]
        for t, (n_cols, max_terms, irp, ici) in enumerate(specs):
            arr[t].n_cols, arr[t].max_terms, arr[t].ind_row_ptr, arr[t].ind_col_idx, arr[t].term_row_ptr = int(n_cols), int(max_terms), _ptr(irp), _ptr(ici), _ptr(rps[t])
        head = (self.handle, nq, _ptr(q_items), int(n_items), arr, len(specs))
        cis, info = self._bounded_rows(arr, len(specs), nq, rps, stats, timing, keep_bounds, lambda: self.lib.urcco_dev_item_bounds(*head),
                                       lambda cis, totals, st: self.lib.urcco_dev_item_rows(*head, _ptr(st)))
        return list(zip(rps, cis)), info

    # ---- device-resident item properties (decision D25; include/urcco.h urcco_dev_props_*) ----
    # The state of a property is three tensors of one entry per item -- t_set int64, pos_set int32, t_unset int64 -- and the store's t_del int64: the bits
    # of the header's unsigned words (torch computes on the signed types), zeros = nothing seen.
    def props_apply(self, n_items: int, items: torch.Tensor, times: torch.Tensor, kinds: Optional[torch.Tensor], pos_base: int, t_set: torch.Tensor,
                    pos_set: torch.Tensor, t_unset: torch.Tensor, n_new: Optional[int] = None):
        """urcco_dev_props_apply: the events at stream positions pos_base .. of one property into its state, in place.  items int32, times int64, kinds
        uint8 (_lib.PROP_SET / PROP_UNSET) or None (all sets); n_new: the events to read (default: all of `items`).  Does not synchronise."""
        n_new = int(items.numel()) if n_new is None else int(n_new)
        self._check(self.lib.urcco_dev_props_apply(self.handle, int(n_items), n_new, _ptr(items), _ptr(times), _ptr(kinds), int(pos_base), _ptr(t_set), _ptr(pos_set),
                                                   _ptr(t_unset)))

    def props_delete(self, n_items: int, items: torch.Tensor, times: torch.Tensor, t_del: torch.Tensor):
        """urcco_dev_props_delete: $delete events (items int32, times int64) into the store's t_del, in place.  Does not synchronise."""
        self._check(self.lib.urcco_dev_props_delete(self.handle, int(n_items), int(items.numel()), _ptr(items), _ptr(times), _ptr(t_del)))

    @staticmethod
    def _prop_state(state) -> "_lib.PropState":
        t_set, pos_set, t_unset, t_del, n_events = state
        return _lib.PropState(_ptr(t_set), _ptr(pos_set), _ptr(t_unset), _ptr(t_del), int(n_events))

    def props_rows(self, n_items: int, state, val_ptr: torch.Tensor, values: torch.Tensor, n_values: int, n_cols: int, keep_bounds: bool = False):
        """urcco_dev_props_bounds + urcco_dev_props_rows: a list-of-strings property as an item x value CSR.  state: (t_set, pos_set, t_unset, t_del | None,
        n_events); val_ptr int64 [n_events + 1] and values int32 [n_values]: the value slice of every stream position.  Returns (row_ptr int64
        [n_items + 1], col_idx int32, info as item_rows gives it): row i = the distinct value ids, ascending, of the winning $set of item i when the
        property is alive.  Reads the bound total between the two calls: one synchronisation."""
        st = self._prop_state(state)
        rp = self.empty(int(n_items) + 1, torch.int64)
        head = (self.handle, int(n_items), C.byref(st), _ptr(val_ptr))
        cis, info = self._bounded_rows(None, 0, int(n_items), [rp], False, False, keep_bounds, lambda: self.lib.urcco_dev_props_bounds(*head, int(n_values), _ptr(rp)),
                                       lambda cis, totals, _st: self.lib.urcco_dev_props_rows(*head, _ptr(values), int(n_values), int(n_cols), _ptr(rp), _ptr(cis[0]),
                                                                                              int(totals[0])))
        return rp, cis[0], info

    def props_dates(self, n_items: int, state, date_values: torch.Tensor) -> torch.Tensor:
        """urcco_dev_props_dates: int64 [n_items], the date of the winning $set (date_values: int64 per stream position) where the property is alive,
        else INT64_MIN.  Does not synchronise."""
        st = self._prop_state(state)
        out = self.empty(max(int(n_items), 1), torch.int64)
        self._check(self.lib.urcco_dev_props_dates(self.handle, int(n_items), C.byref(st), _ptr(date_values), _ptr(out)))
        return out[: int(n_items)]

    def props_exists(self, n_items: int, t_del: torch.Tensor, t_sets) -> torch.Tensor:
        """urcco_dev_props_exists: uint8 [n_items], 0 where the item is deleted -- a $delete that no $set of any of the properties (t_sets: their t_set
        tensors, at most _lib.PROP_MAX) is later than -- else 1: the item_mask of the recommend calls.  Does not synchronise."""
        t_sets = list(t_sets)
        ptrs = (C.c_void_p * max(len(t_sets), 1))(*[t.data_ptr() for t in t_sets])
        out = self.empty(max(int(n_items), 1), torch.uint8)
        self._check(self.lib.urcco_dev_props_exists(self.handle, int(n_items), _ptr(t_del), ptrs, len(t_sets), _ptr(out)))
        return out[: int(n_items)]

    def props_compact(self, n_items: int, state, val_ptr: Optional[torch.Tensor] = None, values: Optional[torch.Tensor] = None, n_values: int = 0,
                      date_values: Optional[torch.Tensor] = None, out=None):
        """urcco_dev_props_compact (decision D28): one property's stream without the values no item's state names any more.  state as in props_rows; a
        list property gives val_ptr / values / n_values, a date property date_values.  Returns (pos_set int32 [n_items], old_pos int32, val_ptr int64 |
        None, values int32 | None, date_values int64 | None, counts int64 [2] = [K, V] on the device): the first K (old_pos, date_values), K + 1
        (val_ptr) and V (values) entries are the result.  out: (val_ptr, values, date_values) tensors to write into, sized by the bounds
        min(n_items, n_events) + 1, n_values and min(n_items, n_events); they must not share memory with the inputs.  Does not synchronise."""
        n_items, n_events, n_values = int(n_items), int(state[4]), int(n_values)
        k_max = min(n_items, n_events)
        st = self._prop_state(state)
        o_vp, o_vals, o_dates = out if out is not None else (None, None, None)
        if val_ptr is not None:
            o_vp = o_vp if o_vp is not None else self.empty(k_max + 1, torch.int64)
            o_vals = o_vals if o_vals is not None else self.empty(max(n_values, 1), torch.int32)
            if o_vp.numel() < k_max + 1 or o_vals.numel() < n_values:
                raise ValueError("props_compact: the output tensors are smaller than min(n_items, n_events) + 1 / n_values")
        if date_values is not None:
            o_dates = o_dates if o_dates is not None else self.empty(max(k_max, 1), torch.int64)
            if o_dates.numel() < k_max:
                raise ValueError("props_compact: the output tensor is smaller than min(n_items, n_events)")
        pos_set = self.empty(max(n_items, 1), torch.int32)
        old_pos = self.empty(max(k_max, 1), torch.int32)
        counts = self.empty(2, torch.int64)
        self._check(self.lib.urcco_dev_props_compact(self.handle, n_items, C.byref(st), _ptr(val_ptr), _ptr(values) if val_ptr is not None else None, n_values,
                                                     _ptr(date_values), _ptr(pos_set), _ptr(old_pos), _ptr(o_vp) if val_ptr is not None else None,
                                                     _ptr(o_vals) if val_ptr is not None else None, _ptr(o_dates) if date_values is not None else None, _ptr(counts)))
        return pos_set, old_pos, o_vp if val_ptr is not None else None, o_vals if val_ptr is not None else None, o_dates if date_values is not None else None, counts

    def _bounded_rows(self, arr, n_types, nq, rps, stats, timing, keep_bounds, bounds, rows):
        """The two-call protocol of history_rows and item_rows.  bounds() leaves in every row_ptr of `rps` the scan of its rows' upper bounds; their
        totals are read (the one synchronisation) and size the col_idx tensors, those of the first n_types go into the struct array `arr`;
        rows(col_idx tensors, totals, stats tensor | None) fills them and rewrites the row_ptr.  Returns (col_idx tensors, info)."""
        ev0 = ev1 = None
        if timing and self.device.type == "cuda":
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record(self.torch_stream)
        self._check(bounds())
        totals = torch.stack([rp[nq] for rp in rps]).cpu().tolist()   # the one synchronisation
        bound_rp = [rp.clone() for rp in rps] if keep_bounds else None
        cis = [self.empty(max(total, 1), torch.int32) for total in totals]
        for t in range(n_types):
            arr[t].term_col_idx, arr[t].term_capacity = _ptr(cis[t]), int(totals[t])
        st = self.empty(_lib.HIST_STATS_LEN, torch.int64) if stats else None
        self._check(rows(cis, totals, st))
        ms = None
        if ev0 is not None:
            ev1.record(self.torch_stream)
            ev1.synchronize()
            ms = ev0.elapsed_time(ev1)
        return cis, {"bounds": totals, "stats": st, "ms": ms, "bound_row_ptr": bound_rp}

    def llr(self, with_a, with_b, with_ab, n_users) -> torch.Tensor:
        out = self.empty(with_a.numel(), torch.float64)
        self._check(self.lib.urcco_dev_llr(self.handle, with_a.numel(), _ptr(with_a), _ptr(with_b), _ptr(with_ab), _ptr(n_users), _ptr(out)))
        return out

    def u01(self, seed: int, row, col, rng: int = _lib.RNG_SPLITMIX53) -> torch.Tensor:
        out = self.empty(row.numel(), torch.float64)
        if rng == _lib.RNG_SPLITMIX53:
            self._check(self.lib.urcco_dev_u01(self.handle, row.numel(), _to_i32(seed), _ptr(row), _ptr(col), _ptr(out)))
        else:
            self._check(self.lib.urcco_dev_u01_rng(self.handle, row.numel(), _to_i32(seed), _ptr(row), _ptr(col), int(rng), _ptr(out)))
        return out


def _to_i32(seed: int) -> int:
    """Scala `Long.toInt` (URAlgorithm.scala:240,325,345)."""
    s = int(seed) & 0xFFFFFFFF
    return s - (1 << 32) if s >= (1 << 31) else s


_TYPESTR = {torch.int32: "<i4", torch.int64: "<i8", torch.float64: "<f8", torch.uint8: "|u1"}
_CTYPE = {torch.int32: C.c_int32, torch.int64: C.c_int64, torch.float64: C.c_double, torch.uint8: C.c_uint8}


class _RawDeviceArray:
    """Zero-copy handle on context-owned device memory (CUDA array interface, which PyTorch-ROCm honours)."""

    def __init__(self, ptr: int, n: int, dtype: torch.dtype):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": _TYPESTR[dtype], "data": (ptr, False), "version": 2}


def _view(ptr: Optional[int], n: int, dtype: torch.dtype, device: torch.device) -> torch.Tensor:
    """Tensor aliasing n elements at a raw pointer of the context (valid until its next build)."""
    if not ptr or n <= 0:
        return torch.empty(0, dtype=dtype, device=device)
    if device.type == "cuda":
        return torch.as_tensor(_RawDeviceArray(ptr, n, dtype), device=device)
    import numpy as np
    return torch.from_numpy(np.ctypeslib.as_array((_CTYPE[dtype] * n).from_address(ptr)))


class Context:
    """urcco_context (include/urcco.h, CONTEXT level): the persistent, multi-stream, multi-GPU form of the model build.

    One context = this process's GPUs [device, device + n_gpus) as ranks [first_rank, first_rank + n_gpus) of a job of
    world_size ranks.  Collectives are RCCL inside the library (nccl_unique_id from `unique_id()` on one rank when the
    ranks are spread over processes) unless `collectives` replaces them (the CPU test-suite: gloo on the simulator)."""

    def __init__(self, device, library=None, n_gpus: int = 1, flags: int = 0, row_rate_mode: int = _lib.ROW_RATE_MAHOUT_INT_DIV,
                 world_size: int = 0, first_rank: int = 0, unique_id: Optional[bytes] = None, collectives=None):
        self.device = torch.device(device)
        self.lib = library if library is not None else _lib.lib()
        index = 0
        if self.device.type == "cuda":
            index = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self.device = torch.device("cuda", index)
        emulate = bool(flags & _lib.FLAG_EMULATE_RANKS)  # measurement only: every rank on the ONE device (include/urcco.h)
        self.devices = [torch.device("cuda", index + (0 if emulate else g)) if self.device.type == "cuda" else self.device for g in range(max(n_gpus, 1))]
        opts = _lib.Options(device=index, row_rate_mode=row_rate_mode, n_gpus=n_gpus, flags=flags)
        comm = None
        self._collectives = collectives
        self._keep = [collectives]
        if world_size or first_rank or unique_id is not None or collectives is not None:
            comm = _lib.CommConfig(world_size=world_size, first_rank=first_rank)
            if unique_id is not None:
                buf = C.create_string_buffer(bytes(unique_id), _lib.UNIQUE_ID_BYTES)
                self._keep.append(buf)
                comm.nccl_unique_id = C.cast(buf, C.c_void_p)
            if collectives is not None:
                comm.collectives = C.pointer(collectives.struct)
        handle = C.c_void_p()
        _lib.check(self.lib.urcco_context_create(C.byref(opts), C.byref(comm) if comm is not None else None, C.byref(handle)), self.lib)
        self.handle = handle
        self.n_local = int(self.lib.urcco_context_local_gpus(handle))
        self.devices = self.devices[: self.n_local] if len(self.devices) >= self.n_local else [torch.device("cuda", index + g) for g in range(self.n_local)]
        self._last = None

    @staticmethod
    def unique_id(library=None) -> bytes:
        lib = library if library is not None else _lib.lib()
        buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
        _lib.check(lib.urcco_comm_unique_id(buf), lib)
        return buf.raw

    def collectives_error(self):
        return getattr(self._collectives, "error", None)

    def _check(self, status: int):
        if status != _lib.OK and self.collectives_error() is not None:
            raise self.collectives_error()      # the Python exception behind a failed collectives callback
        _lib.check(status, self.lib)

    def close(self):
        if self.handle:
            self.lib.urcco_context_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._check(self.lib.urcco_context_synchronize(self.handle))

    def set_timing(self, enable: bool):
        self._check(self.lib.urcco_context_set_timing(self.handle, int(enable)))

    def set_debug(self, flags: int):
        self._check(self.lib.urcco_context_set_debug(self.handle, int(flags)))

    def set_flags(self, flags: int):
        self._check(self.lib.urcco_context_set_flags(self.handle, int(flags)))

    def get_timings(self):
        ms = (C.c_double * _lib.N_STAGES)()
        n = (C.c_int64 * _lib.N_STAGES)()
        self._check(self.lib.urcco_context_get_timings(self.handle, ms, n))
        return {_lib.STAGE_NAMES[i]: (ms[i], n[i]) for i in range(_lib.N_STAGES) if _lib.STAGE_NAMES[i]}

    def get_timings_gpu(self, local_gpu: int):
        """The stage timings of ONE local GPU (rank first_rank + local_gpu)."""
        ms = (C.c_double * _lib.N_STAGES)()
        n = (C.c_int64 * _lib.N_STAGES)()
        self._check(self.lib.urcco_context_get_timings_gpu(self.handle, int(local_gpu), ms, n))
        return {_lib.STAGE_NAMES[i]: (ms[i], n[i]) for i in range(_lib.N_STAGES) if _lib.STAGE_NAMES[i]}

    def build(self, shards: Sequence[Sequence[DevCsr]], params: Sequence[DatasetParams], seed: int, n_users_total: Optional[int] = None,
              row_bases: Optional[Sequence[int]] = None, input_stream=None):
        """Enqueue one model build.  shards[d][g] = event type d's user rows held by local GPU g (shards[d] may also be a
        single DevCsr for a one-GPU context).  Returns immediately (after the one blocking read of ranges / sizes with
        more than one rank); read the outcome with results()."""
        n_ds = len(shards)
        if n_ds == 0 or n_ds != len(params):
            raise ValueError("need one DatasetParams per matrix and at least the primary matrix")
        per = [list(sd) if isinstance(sd, (list, tuple)) else [sd] for sd in shards]
        L = self.n_local
        if any(len(p) != L for p in per):
            raise ValueError(f"every event type needs one shard per local GPU ({L})")
        if row_bases is None:
            row_bases, acc = [], 0
            for g in range(L):
                row_bases.append(acc)
                acc += per[0][g].n_rows
        if n_users_total is None:
            n_users_total = sum(m.n_rows for m in per[0])
        ds = (_lib.DevDataset * n_ds)()
        keep = []
        for d in range(n_ds):
            arr = (_lib.DevShard * L)()
            for g, m in enumerate(per[d]):
                arr[g].n_rows, arr[g].row_base, arr[g].nnz = m.n_rows, row_bases[g], m.nnz_bound
                arr[g].row_ptr, arr[g].col_idx = m.row_ptr.data_ptr(), m.col_idx.data_ptr()
            keep.append(arr)
            p = params[d]
            ds[d].n_cols = per[d][0].n_cols
            ds[d].max_elements_per_row, ds[d].max_interesting_elements = p.max_elements_per_row, p.max_interesting_elements
            ds[d].has_min_llr, ds[d].min_llr = int(p.min_llr is not None), float(p.min_llr) if p.min_llr is not None else 0.0
            ds[d].shards = arr
        out = (_lib.DevResult * (n_ds * L))()
        st = None
        if input_stream is not None:
            st = C.c_void_p(input_stream.cuda_stream)
        elif self.device.type == "cuda" and L == 1:
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        self._check(self.lib.urcco_context_build_device(self.handle, ds, n_ds, int(n_users_total), _to_i32(seed), st, out))
        self._last = (out, n_ds, [p.max_interesting_elements for p in params], [per[d][0].n_cols for d in range(n_ds)], (per, keep))
        return out

    def wait(self):
        """torch's current stream waits (on the device) for the last build (single-GPU contexts)."""
        if self.device.type == "cuda" and self.n_local == 1:
            self._check(self.lib.urcco_context_wait_stream(self.handle, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        else:
            self.synchronize()

    def results(self) -> List[List[DevIndicators]]:
        """Views on the last build's outputs (context-owned memory, valid until the next build): [event type][local GPU].
        Synchronises."""
        self.synchronize()
        out, n_ds, ks, n_cols, _ = self._last
        L = self.n_local
        res = []
        for d in range(n_ds):
            row = []
            for g in range(L):
                r = out[d * L + g]
                dev = self.devices[g]
                n = r.item_hi - r.item_lo
                s_rp = _view(r.sampled_row_ptr, r.sampled_rows + 1, torch.int64, dev)
                s_nnz = int(s_rp[-1]) if s_rp.numel() else 0
                s_ci = _view(r.sampled_col_idx, max(s_nnz, 1), torch.int32, dev)
                if r.sampled_col_mask != -1:   # a sharded build's rows arrive with their columns' counts above the column bits (include/urcco.h)
                    s_ci = s_ci & int(r.sampled_col_mask)
                row.append(DevIndicators(r.item_lo, r.item_hi, n_cols[d], ks[d], _view(r.row_ptr, n + 1, torch.int64, dev),
                                         _view(r.col_idx, max(n * ks[d], 1), torch.int32, dev), _view(r.llr, max(n * ks[d], 1), torch.float64, dev),
                                         _view(r.stats, _lib.STATS_LEN, torch.int64, dev), s_rp, s_ci,
                                         int(r.sampled_nnz_total)))
            res.append(row)
        return res


def cross_occurrence_context(ctx: Context, mats: Sequence[DevCsr], params: Sequence[DatasetParams], seed: int) -> List[DevIndicators]:
    """SimilarityAnalysis.crossOccurrenceDownsampled on a one-GPU context: one build, results as views."""
    ctx.build([[m] for m in mats], params, seed)
    return [r[0] for r in ctx.results()]


def cross_occurrence_device(sess: DeviceSession, mats: Sequence[DevCsr], params: Sequence[DatasetParams], seed: int,
                            row_rate_mode: int = _lib.ROW_RATE_MAHOUT_INT_DIV, item_lo: int = 0,
                            item_hi: Optional[int] = None) -> List[DevIndicators]:
    """SimilarityAnalysis.crossOccurrenceDownsampled on one GPU, inputs and outputs in HBM, no host sync.
    mats[0] is the primary matrix A; returns the indicator matrices for A'A, A'B_1, ..."""
    if len(mats) == 0 or len(mats) != len(params):
        raise ValueError("need one DatasetParams per matrix and at least the primary matrix")
    a_raw = mats[0]
    for m in mats:
        if m.n_rows != a_raw.n_rows:
            raise ValueError("all matrices share the user dictionary: row counts differ")
    if item_hi is None:
        item_hi = a_raw.n_cols
    raw = sess.column_counts(a_raw.col_idx, a_raw.nnz_bound, a_raw.n_cols)
    a, cnt_a = sess.downsample(a_raw, a_raw.nnz_bound, raw, seed, params[0].max_elements_per_row, row_rate_mode)
    a_col_ptr, a_row_idx = sess.transpose(a, cnt_a)
    out = []
    for d, (m, p) in enumerate(zip(mats, params)):
        if d == 0:
            b, cnt_b = a, cnt_a
        else:
            raw_b = sess.column_counts(m.col_idx, m.nnz_bound, m.n_cols)
            b, cnt_b = sess.downsample(m, m.nnz_bound, raw_b, seed, p.max_elements_per_row, row_rate_mode)
        out.append(sess.cco_rows(item_lo, item_hi, a_raw.n_cols, a_col_ptr, a_row_idx, a.nnz_bound, b, cnt_a, cnt_b, a_raw.n_rows, d == 0, p))
    return out
