"""The problem and the check of the sort + unique row unit (csrc/cco_sorted_rows.h) as the CSR build reaches it, shared by test_sim_sorted_rows.py
and test_gpu_sorted_rows.py: one call of ingest.csr_from_pairs over a shuffled pair stream whose rows sit on every class edge of the unit (one wave up
to 64 raw entries, one block in LDS up to 4096, the padded network in global memory beyond), compared exactly with np.unique per row."""
import functools

import numpy as np
import torch

SENT = 0x7fffffff                 # the unit's "no column": an ordinary column to the CSR build, which drops nothing but duplicates
LENGTHS = [0, 1, 63, 64, 65, 256, 257, 4095, 4096, 4097, 8193]   # raw entries: the class edges, and one non-power-of-two above the LDS limit
CLASS_LENGTHS = [(40, 50), (300, 500), (4200, 4100)]             # per class (wave, LDS, global): (all entries equal, the sentinel row)
N_SKIPPED = 300                   # pairs of each skipped kind: row < 0, col < 0, both
N_COLS = 1 << 31                  # column ids are any non-negative int32


@functools.lru_cache(maxsize=None)
def problem():
    """Returns (rows int32 [n], cols int32 [n], n_rows, want_row_ptr int64 [n_rows + 1], want_col_idx int32 [nnz]): the stream and np.unique per row."""
    rng = np.random.default_rng(20265)
    raw = []
    for L in LENGTHS:
        if L < 63:
            raw.append(rng.integers(0, 1000, L))
            continue
        raw.append(rng.integers(0, L // 2, L))                              # many duplicates
        raw.append(rng.permutation(4 * L)[:L] * 3 + 5)                      # all distinct
    for n_equal, n_sent in CLASS_LENGTHS:
        raw.append(np.full(n_equal, 123456))
        r = rng.integers(0, 100000, n_sent)
        r[[n_sent // 3, n_sent - 2]] = SENT                                 # twice, in the middle of ordinary columns
        raw.append(r)
    assert all(r.size == 0 or (r.min() >= 0 and r.max() <= SENT) for r in raw)
    n_rows = len(raw) + 5                                                   # a few rows no pair names
    ids = rng.permutation(n_rows)[: len(raw)]
    want = [np.zeros(0, np.int64)] * n_rows
    for i, r in zip(ids, raw):
        want[i] = np.unique(r)
    rows = np.concatenate([np.full(r.size, i, np.int64) for i, r in zip(ids, raw)])
    cols = np.concatenate(raw).astype(np.int64)
    skip_r = np.concatenate([rng.integers(-5, 0, N_SKIPPED), rng.integers(0, n_rows, N_SKIPPED), rng.integers(-5, 0, N_SKIPPED)])
    skip_c = np.concatenate([rng.integers(0, 1000, N_SKIPPED), rng.integers(-5, 0, N_SKIPPED), rng.integers(-5, 0, N_SKIPPED)])
    rows, cols = np.concatenate([rows, skip_r]), np.concatenate([cols, skip_c])
    order = rng.permutation(rows.size)
    want_rp = np.zeros(n_rows + 1, np.int64)
    np.cumsum([w.size for w in want], out=want_rp[1:])
    return rows[order].astype(np.int32), cols[order].astype(np.int32), n_rows, want_rp, np.concatenate(want).astype(np.int32)


def run(sess):
    """One call: (row_ptr, col_idx[:nnz], nnz) on the host."""
    from universal_recommender_amd import ingest
    rows, cols, n_rows, _, _ = problem()
    m = ingest.csr_from_pairs(sess, torch.from_numpy(rows).to(sess.device), torch.from_numpy(cols).to(sess.device), n_rows, N_COLS)
    sess.synchronize()
    return m.row_ptr.cpu().numpy(), m.col_idx.cpu().numpy()[: m.nnz_bound], m.nnz_bound


def check(sess):
    rows, _, n_rows, want_rp, want_ci = problem()
    assert 40000 <= rows.size <= 60000, rows.size
    rp, ci, nnz = run(sess)
    assert rp.shape == (n_rows + 1,) and np.array_equal(rp, want_rp)
    assert nnz == want_rp[-1]
    assert np.array_equal(ci, want_ci)
    rp2, ci2, nnz2 = run(sess)                                              # the same session again: scratch left by the first call does not matter
    assert nnz2 == nnz and np.array_equal(rp2, rp) and np.array_equal(ci2, ci)
