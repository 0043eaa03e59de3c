"""THE PRODUCTION FORM OF THE MICRO CLASS (-m gpu).  conftest.py sets URCCO_MICRO_SPLIT_ROWS=0 for this process and the library reads it once,
so every other GPU test runs the micro class split into its three sub-lists.  Builds below 1,000,000 item rows keep ONE list by default --
BASELINE configs 1, 2 and 3, every rank of an 8-rank build, what bench.py times.  Each test here starts tests/production_forms_child.py in a
fresh process WITHOUT the variable (one child at a time, parent + child = two GPU processes; this process opens no session of its own) and
re-asserts from the child's JSON lines what names the form: stats[31] (rows binned into the two shared-wave sub-lists) against the item rows
of each build.  A child that timed out or died of a signal may have left the GPU faulted: the pytest session ends there."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "production_forms_child.py")
SPLIT_ROWS = 1_000_000
# Seconds: three times the test's wall time measured once on an MI355X box (edges 2.6 s, config3 7.8 s, ranks8 17.3 s, threshold 18.7 s; oracle
# already built), rounded up to the next 30 s -- for a cold oracle build and the slower hosts of the pool (the oracle's CPU leg varies 73 to
# 82 M pairs/s between boxes).
TIMEOUT = {"edges": 30, "config3": 30, "ranks8": 60, "threshold": 60}
FAULT_CODES = (124, 134, 137, 139)


def run_group(group):
    torch.cuda.empty_cache()
    env = {k: v for k, v in os.environ.items() if k != "URCCO_MICRO_SPLIT_ROWS"}     # NOT set to the default's value: the library's own constant is read
    try:
        r = subprocess.run([sys.executable, CHILD, group], env=env, capture_output=True, text=True, timeout=TIMEOUT[group])
    except subprocess.TimeoutExpired as e:
        out = (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        err = (e.stderr or b"").decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.exit(f"production_forms_child.py {group} ran into its {TIMEOUT[group]} s limit; the GPU may be hung, no further test is started\n{out[-3000:]}\n{err[-3000:]}", returncode=3)
    tail = r.stdout[-6000:] + "\n" + r.stderr[-4000:]
    if r.returncode < 0 or r.returncode in FAULT_CODES:
        pytest.exit(f"production_forms_child.py {group} died with status {r.returncode}; the GPU may be faulted, no further test is started\n{tail}", returncode=3)
    assert r.returncode == 0, tail
    assert r.stdout.rstrip().splitlines()[-1] == f"PRODUCTION_FORMS_OK {group}", tail
    print(r.stdout)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    builds = [l for l in lines if "item_rows" in l]
    assert builds, tail
    for b in builds:
        assert len(b["shared_wave_rows"]) == len(b["rows_by_class"]) == len(b["pairs"]) > 0, b
        if b["item_rows"] < SPLIT_ROWS:
            assert all(x == 0 for x in b["shared_wave_rows"]), b         # one list
        else:
            assert all(x > 0 for x in b["shared_wave_rows"]), b          # split
    return builds, lines


def test_edges_one_list():
    builds, lines = run_group("edges")
    assert all(b["item_rows"] < SPLIT_ROWS for b in builds)
    cases = [l for l in lines if "case" in l]
    assert len(cases) == 9 and all(c["micro_rows"] > 0 for c in cases), cases


def test_config3_one_list():
    builds, _ = run_group("config3")
    assert len(builds) == 1 and builds[0]["item_rows"] == 200_000 and sum(builds[0]["pairs"]) == 90668283
    assert all(rows[0] > 0 for rows in builds[0]["rows_by_class"]), builds[0]


def test_eight_ranks_one_list_each():
    builds, _ = run_group("ranks8")
    one = [b for b in builds if b["item_rows"] >= SPLIT_ROWS]
    ranks = [b for b in builds if b["item_rows"] < SPLIT_ROWS]
    assert len(one) == 1 and one[0]["item_rows"] == 2_000_000 and len(ranks) == 8 and sum(b["item_rows"] for b in ranks) == 2_000_000
    assert all(sum(rows[0] for rows in b["rows_by_class"]) > 0 for b in ranks)
    assert sum(sum(b["pairs"]) for b in ranks) == sum(one[0]["pairs"])


def test_threshold_both_sides():
    builds, _ = run_group("threshold")
    assert [b["item_rows"] for b in builds] == [999_999, 1_000_000, 999_999, 999_999]
    assert all(b["pairs"] == builds[0]["pairs"] for b in builds[:3])
    assert all(b["rows_by_class"] == builds[0]["rows_by_class"] for b in builds[:3])
