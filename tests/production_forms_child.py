"""Helper of tests/test_gpu_production_forms.py -- a plain script, not collected by pytest: the library AT ITS DEFAULTS on cuda:0.

tests/conftest.py lowers the threshold of the micro class's split (URCCO_MICRO_SPLIT_ROWS=0, read once by the library) for the whole pytest
process, so every -m gpu test runs the split form: three sub-lists, rows of <= 16 / <= 32 pairs and users four / two to a wave.  Builds of
fewer than 1,000,000 item rows -- BASELINE configs 1, 2 and 3, every rank of an 8-rank build, what bench.py times -- keep ONE list in
production: every micro row, down to a row of one pair, goes through cco_rows_micro_kernel<64>.  This process never imports conftest and
refuses to start with the variable set; it runs one group of builds (argv[1]) in the form the library itself chooses and compares every build
with the C oracle through the checkers of the suite (helpers.compare_with_oracle, compare_with_oracle_large, check_indicators: ids exact
except ties at the k-th score, |dLLR| <= LLR_TOL, pairs equal, overflow word 0; the large checker also the down-sampled matrices bit for bit).
Which form ran is asserted through stats[STATS_LEN - 1], the rows binned into the two shared-wave sub-lists (0 = one list).

Groups: edges | config3 | ranks8 | threshold.  Per build one JSON line (name, item rows, rows per accumulator class, stats[31], pairs,
rows that needed the k-boundary tie rule -- lists over the build's event types; a multi-rank build: one line per rank); the last line is
PRODUCTION_FORMS_OK <group>."""
import json
import os
import sys

assert "URCCO_MICRO_SPLIT_ROWS" not in os.environ, "this process checks the library's OWN threshold: start it without URCCO_MICRO_SPLIT_ROWS"

try:  # a GPU fault aborts the process: no core dump of a process with tens of GB mapped (as conftest.py)
    import resource
    resource.setrlimit(resource.RLIMIT_CORE, (0, 0))
except Exception:
    pass

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import helpers
from oracle import c_oracle as O
from universal_recommender_amd import _lib

SPLIT_ROWS = 1_000_000       # micro_split_for (csrc/cco_rows.hip): the library's default, re-stated only to say what each build must report
W31 = _lib.STATS_LEN - 1
OVERFLOW = 1 + 4 * _lib.N_BINS
BUILDS = []                  # every build of this process: (name, item rows, [stats vector per event type], [tie rows per event type])


def P(max_rows=500, k=50, min_llr=None):
    return O.DatasetParams(max_rows, k, min_llr)


def record(name, item_rows, stats, ties):
    stats = [np.asarray(s) for s in stats]
    BUILDS.append((name, int(item_rows), stats, list(ties)))
    print(json.dumps({"name": name, "item_rows": int(item_rows), "rows_by_class": [[int(x) for x in s[1:8]] for s in stats],
                      "shared_wave_rows": [int(s[W31]) for s in stats], "pairs": [int(s[0]) for s in stats], "tie_rows": [int(t) for t in ties]}), flush=True)


def assert_form(name, item_rows, stats, shared_ref=None):
    """One list below the threshold: the word is 0.  At or above it: the numpy count of the two shared-wave sub-lists (shared_ref, per event type)
    where the caller has one, else above 0."""
    for d, s in enumerate(stats):
        if item_rows < SPLIT_ROWS:
            assert int(s[W31]) == 0, f"{name}, event {d}: {item_rows} item rows must keep the micro class as one list, stats[{W31}] = {int(s[W31])}"
        elif shared_ref is not None:
            assert int(s[W31]) == shared_ref[d], f"{name}, event {d}: stats[{W31}] = {int(s[W31])}, the shared-wave sub-lists hold {shared_ref[d]} rows"
        else:
            assert int(s[W31]) > 0, f"{name}, event {d}: {item_rows} item rows must split the micro class, stats[{W31}] = 0"


def recording_compare(name):
    """helpers.compare_with_oracle, every call's statistics recorded (the case functions do not return them) and its form asserted."""
    def compare(sess, mats, params, seed, mode=0, item_lo=0, item_hi=None, exact_ids=False):
        out, ref, stats = helpers.compare_with_oracle(sess, mats, params, seed, mode, item_lo, item_hi, exact_ids)
        n = (mats[0].n_cols if item_hi is None else item_hi) - item_lo
        record(name, n, [s[0] for s in stats], [s[2] for s in stats])
        assert_form(name, n, [s[0] for s in stats])
        return out, ref, stats
    return compare


# ---- edges ---------------------------------------------------------------------------------------------------------------------------
EXACT_PAIRS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64]


def exact_pairs_case(b_cols=300):
    """Item rows of EXACTLY p pairs, p in EXACT_PAIRS, built by hand: held by one user whose B row has p columns (cA = 1), or by p users of one
    column each (cA = p) -- p distinct columns, one column p times (k11 = p, one candidate), or two columns in turn.  Each user of A holds one
    item; three copies of every form with other column strides (7, 11, 13: coprime to b_cols, so p <= 64 columns stay distinct); 40 users
    without a primary event give the columns different counts.  In the one-list form each of these rows has a wave to itself: 1 .. 64 of its
    lanes hold a pair.  Returns (A, B, pairs per item, cA per item)."""
    a_item, b_rows, pairs, ca = [], [], [], []
    item = 0
    for p in EXACT_PAIRS:
        for stride in (7, 11, 13):
            for form in ["one_user"] + (["distinct", "same", "two"] if p > 1 else []):
                base = item * 17
                if form == "one_user":
                    a_item.append(item)
                    b_rows.append(np.unique([(base + j * stride) % b_cols for j in range(p)]))
                    ca.append(1)
                else:
                    for j in range(p):
                        a_item.append(item)
                        col = (base + j * stride) % b_cols if form == "distinct" else (base % b_cols if form == "same" else (base + (j % 2) * stride) % b_cols)
                        b_rows.append(np.array([col]))
                    ca.append(p)
                pairs.append(p)
                item += 1
    n_prim = len(a_item)
    for t in range(40):
        b_rows.append(np.unique([(t * 5 + q * 29) % b_cols for q in range(6)]))
    n_users = len(b_rows)
    a_rp = np.concatenate([np.arange(n_prim + 1, dtype=np.int64), np.full(n_users - n_prim, n_prim, np.int64)])
    a = O.Csr(n_users, item, a_rp, np.asarray(a_item, np.int32))
    b_rp = np.zeros(n_users + 1, np.int64)
    np.cumsum([r.size for r in b_rows], out=b_rp[1:])
    b = O.Csr(n_users, b_cols, b_rp, np.concatenate(b_rows).astype(np.int32))
    return a, b, np.asarray(pairs), np.asarray(ca)


def exact_pairs_sweep(sess):
    a, b, pairs, ca = exact_pairs_case()
    users = np.repeat(np.arange(a.n_rows), np.diff(a.row_ptr))
    w = np.bincount(a.col_idx, weights=np.diff(b.row_ptr)[users].astype(np.float64), minlength=a.n_cols).astype(np.int64)
    assert np.array_equal(w, pairs) and np.array_equal(np.bincount(a.col_idx, minlength=a.n_cols), ca), "the hand-built rows do not have the pairs they are named for"
    assert all(((pairs == p) & (ca == 1)).any() and ((pairs == p) & (ca == p)).any() for p in EXACT_PAIRS)
    compare = recording_compare("exact_pairs_sweep")
    for k in (1, 3, 50):
        _, _, stats = compare(sess, [a, b], [P(100000, k), P(100000, k)], 29)
        assert int(stats[1][0][1]) == a.n_cols, (stats[1][0][1:8], a.n_cols)     # A'B: every item row is a micro row
        assert int(stats[0][0][1]) == a.n_cols, stats[0][0][1:8]                 # A'A: w = cA <= 64 (rows of self pairs only: empty indicator rows)


def group_edges(sess):
    """The small cases of the suite as builds of their production form: on hardware their micro rows have only met the split kernels.
    Every case must hold micro rows in at least one of its builds (test_all_equal_llr_ties_cut_by_column through its micro-class block)."""
    import test_gpu_parity as parity
    import test_sim_kernel_logic as logic
    cases = [(logic, f) for f in (logic.test_micro_class_every_ranking_form, logic.test_small_three_events_all_modes, logic.test_empty_and_ragged_inputs,
                                  logic.test_item_range_slices_concatenate, logic.test_all_equal_llr_ties_cut_by_column,
                                  logic.test_counts_aboard_and_the_count_gather_agree)]
    cases += [(parity, parity.test_config1_handmade), (parity, parity.test_config2_movielens), (None, exact_pairs_sweep)]
    without = []
    for module, case in cases:
        first = len(BUILDS)
        if module is not None:
            original = module.compare_with_oracle
            module.compare_with_oracle = recording_compare(case.__name__)      # what the case asserts is untouched: the same checker, its statistics kept
            try:
                case(sess)
            finally:
                module.compare_with_oracle = original
        else:
            case(sess)
        mine = BUILDS[first:]
        assert mine, f"{case.__name__} built nothing through compare_with_oracle"
        micro_rows = sum(int(s[1]) for _, _, stats, _ in mine for s in stats)
        print(json.dumps({"case": case.__name__, "builds": len(mine), "micro_rows": micro_rows}), flush=True)
        assert all(int(s[W31]) == 0 for _, _, stats, _ in mine for s in stats)
        if micro_rows == 0:
            without.append(case.__name__)
    # every case has been compared with the oracle by now; a case without a single micro row says nothing about the one-list form
    assert not without, f"no row of the micro class in any build of: {', '.join(without)}"


# ---- config3 -------------------------------------------------------------------------------------------------------------------------
CONFIG3_MIN_SHARE_LE32 = 0.10   # of the micro rows of every event type: rows of <= 32 pairs and users, which only the one-list form sends through <64>


def group_config3(sess):
    """BASELINE config 3 at full size (1M x 200K, 3 event types, the seed of bench.py and of test_full_config3_every_row), every row."""
    import test_gpu_scale as scale
    import test_sim_kernel_logic as logic
    from universal_recommender_amd import synth
    mats = scale._mats(synth.config3(1.0))
    params = [P(), P(), P()]
    _, res = helpers.compare_with_oracle_large(sess, mats, params, 20260925)
    stats = [st for st, _ in res]
    n = mats[0].n_cols
    record("config3", n, stats, [t for _, t in res])
    assert sum(int(st[0]) for st in stats) == 90668283           # the pairs figure bench.py reports for this seed
    assert n < SPLIT_ROWS
    assert_form("config3", n, stats)
    ref = logic.micro_sub_range_rows_of_build(mats, params, 20260925)
    for d, (st, (r16, r32, r64)) in enumerate(zip(stats, ref)):
        assert int(st[1]) == r16 + r32 + r64, (d, st[1:8], r16, r32, r64)
        share = (r16 + r32) / max(r16 + r32 + r64, 1)
        print(json.dumps({"name": "config3", "event": d, "micro_rows_le16": r16, "micro_rows_le32": r32, "micro_rows_le64": r64, "share_le32": round(share, 4)}), flush=True)
        assert share >= CONFIG3_MIN_SHARE_LE32, f"event {d}: only {share:.4f} of the micro rows have <= 32 pairs and users: the <64> kernels met too few of them"


# ---- ranks8 --------------------------------------------------------------------------------------------------------------------------
def group_ranks8(sess):
    """Config 5 with 2.5M users x the full item spaces: the one-rank build (2M item rows: split) and eight emulated ranks (about 250K item rows each,
    the rows per rank of bench.py --emulate-ranks 8: one list), every row of both against one oracle pass."""
    import test_gpu_scale as scale
    res, res8 = scale.config5_one_rank_and_eight_ranks(sess, 0.25)
    stats = [st for st, _ in res]
    record("config5_quarter_one_rank", 2_000_000, stats, [t for _, t in res])
    assert_form("config5_quarter_one_rank", 2_000_000, stats)
    W = len(res8[0])
    assert W == 8
    for g in range(W):
        n = res8[0][g].item_hi - res8[0][g].item_lo
        assert all(row[g].item_hi - row[g].item_lo == n for row in res8) and 0 < n < SPLIT_ROWS, (g, n)
        rank_stats = [row[g].stats for row in res8]
        record(f"config5_quarter_rank{g}_of_8", n, rank_stats, [-1] * len(rank_stats))     # (-1: the checker counts tie rows over the ranks together)
        assert_form(f"rank {g} of 8", n, rank_stats)
        assert all(int(s[OVERFLOW]) == 0 for s in rank_stats)
        assert sum(int(s[1]) for s in rank_stats) > 0, f"rank {g}: no row of the micro class"
    assert sum(res8[0][g].item_hi - res8[0][g].item_lo for g in range(W)) == 2_000_000
    ratio, work = scale.ranks_work_imbalance(res8)
    print(json.dumps({"name": "config5_quarter_8_ranks", "work_max_over_mean": round(float(ratio), 4), "pairs_by_rank": [int(x) for x in work]}), flush=True)
    assert ratio < 1.05, work


# ---- threshold -----------------------------------------------------------------------------------------------------------------------
NO_CUT = 10_000_000   # maxElementsPerRow / interaction cut above every row length and column count of the threshold workload


def group_threshold(sess):
    """The switch itself: the same interactions as a catalogue of 999,999 item rows (one list), of 1,000,000 (one empty row more: split -- both widths
    take 20 column bits, only the form changes) and as two ranges of 999,999 rows cut from the 1,000,000 (one list: the binning pass and the
    launch of the row kernels must agree on the range's length, or two sub-lists are filled and never launched).
    The workload is one that nothing is down-sampled in: no user row exceeds 25 entries, and the interaction cut is set above every column's
    count (the default of 500 would thin the hot columns of both matrices), so the rows per size range are those of the raw matrices.  Against a
    vacuous run every size range must hold 100,000 rows per event type (50,000: the <= 64 remainder of A'B)."""
    import test_sim_kernel_logic as logic
    rng = np.random.default_rng(1000000)
    a = helpers.rand_csr(rng, 300_000, 999_999, 8, zipf_s=0.6)
    b = helpers.rand_csr(rng, 300_000, 50_000, 6, zipf_s=1.0)
    a1m = O.Csr(a.n_rows, 1_000_000, a.row_ptr, a.col_idx)
    params, seed = [P(NO_CUT), P(NO_CUT)], 1000000
    assert max(int(np.diff(m.row_ptr).max()) for m in (a, b)) <= 25 and max(int(O.column_counts(m).max()) for m in (a, b)) <= NO_CUT
    assert all(O.downsample(m, O.column_counts(m), seed, NO_CUT).nnz == m.nnz for m in (a, b)), "the workload must not be down-sampled"
    ref = logic.micro_sub_range_rows_of_build([a1m, b], params, seed)
    print(json.dumps({"name": "threshold", "micro_rows_le16_le32_le64": ref}), flush=True)
    builds = [("threshold_a_999999", [a, b], 0, 999_999), ("threshold_b_1000000", [a1m, b], 0, 1_000_000),
              ("threshold_c_range_0_999999", [a1m, b], 0, 999_999), ("threshold_d_range_1_1000000", [a1m, b], 1, 1_000_000)]
    hosts = []
    for name, mats, lo, hi in builds:
        out, _, stats = helpers.compare_with_oracle(sess, mats, params, seed, 0, lo, hi)
        record(name, hi - lo, [s[0] for s in stats], [s[2] for s in stats])
        assert_form(name, hi - lo, [s[0] for s in stats], shared_ref=[r[0] + r[1] for r in ref])
        rows_here = logic.micro_sub_range_rows_of_build(mats, params, seed, 0, lo, hi)
        for d, s in enumerate(stats):
            assert int(s[0][1]) == sum(rows_here[d]), (name, d, s[0][1:8], rows_here[d])
        hosts.append([o.to_host() for o in out])
        del out
    # the forms against each other: rows 0 .. 999,998 of (a), (b), (c) and rows 1 .. 999,998 of (d) -- lengths and ids exact, LLR bit for bit
    ha, hb, hc, hd = hosts
    for d in range(2):
        rp, ci, llr = ha[d]
        e = int(rp[999_999])
        for label, (rp2, ci2, llr2) in (("(b) 1,000,000 rows, split", hb[d]), ("(c) range [0, 999,999)", hc[d])):
            assert np.array_equal(rp, rp2[:1_000_000]), f"event {d}: row lengths of (a) and {label} differ"
            assert np.array_equal(ci, ci2[:e]), f"event {d}: ids of (a) and {label} differ"
            assert np.array_equal(llr.view(np.int64), llr2[:e].view(np.int64)), f"event {d}: LLR bits of (a) and {label} differ"
        assert int(hb[d][0][1_000_000]) == e, "the added item row of (b) is not empty"
        rp2, ci2, llr2 = hd[d]
        s = int(rp[1])
        assert np.array_equal(rp[1:] - s, rp2[:999_999]) and int(rp2[999_999]) == e - s, f"event {d}: row lengths of (a) and (d) range [1, 1,000,000) differ"
        assert np.array_equal(ci[s:e], ci2[:e - s]), f"event {d}: ids of (a) and (d) differ"
        assert np.array_equal(llr[s:e].view(np.int64), llr2[:e - s].view(np.int64)), f"event {d}: LLR bits of (a) and (d) differ"
    print(json.dumps({"name": "threshold", "forms_agree": "lengths, ids and LLR bits of (a), (b), (c), (d)"}), flush=True)
    for d, r in enumerate(ref):          # not vacuous: every size range of both event types well filled
        assert r[0] >= 100_000 and r[1] >= 100_000 and r[2] >= (100_000 if d == 0 else 50_000), f"event {d}: rows per size range {r}"


GROUPS = {"edges": group_edges, "config3": group_config3, "ranks8": group_ranks8, "threshold": group_threshold}


def main():
    group = sys.argv[1] if len(sys.argv) > 1 else ""
    assert group in GROUPS, f"usage: production_forms_child.py {' | '.join(GROUPS)}"
    from universal_recommender_amd.device import DeviceSession
    assert torch.cuda.is_available(), "needs a HIP device"
    assert os.path.exists(_lib.DEFAULT_PATH), f"{_lib.DEFAULT_PATH} is missing: build the library first (__graft_entry__.build)"
    sess = DeviceSession(torch.device("cuda", 0), _lib.load(_lib.DEFAULT_PATH))
    try:
        GROUPS[group](sess)
    finally:
        sess.close()
    assert BUILDS and "conftest" not in sys.modules and "URCCO_MICRO_SPLIT_ROWS" not in os.environ
    free, total = torch.cuda.mem_get_info()
    print(json.dumps({"group": group, "builds": len(BUILDS), "peak_torch_gpu_bytes": int(torch.cuda.max_memory_allocated()),
                      "device_bytes_in_use_at_exit": int(total - free)}), flush=True)
    print(f"PRODUCTION_FORMS_OK {group}", flush=True)


if __name__ == "__main__":
    main()
