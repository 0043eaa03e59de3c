"""The small-row body with eight pairs and two users per lane (csrc/cco_rows.hip, cco_rows_small_kernel<8, 2>) on hardware: the cases of
tests/block_small_wave_cases.py -- each compared with the oracle and, bit for bit, with the same build under NO_BLOCK_SMALL_WAVE; COUNT_BLOCK_SMALL_WAVE
against the model, per list --, one realistic mix, and the production default (no URCCO_MICRO_SPLIT_ROWS) in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import block_small_wave_cases as C
from oracle import c_oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_user_count_boundaries_with_empty_rows(gpu_session):
    C.case_user_boundaries(gpu_session)


def test_pair_count_boundaries(gpu_session):
    C.case_pair_boundaries(gpu_session)


def test_survivor_counts_around_64(gpu_session):
    C.case_survivor_counts(gpu_session)


def test_fallback_shapes(gpu_session):
    C.case_fallback_shapes(gpu_session)


@pytest.mark.parametrize("k", [1, 7, 50, 63, 64, 65])
def test_k_domain(gpu_session, k):
    C.case_k(gpu_session, k)


def test_min_llr_removes_part_of_a_row(gpu_session):
    C.case_min_llr(gpu_session)


def test_self_pair_mixed_sizes_and_unordered_rows(gpu_session):
    C.case_self_pair_and_unordered(gpu_session, gpu_session.lib)


def test_column_addressed_accumulator(gpu_session):
    C.case_column_addressed(gpu_session)


def test_packed_and_plain_forms_agree(gpu_session):
    C.case_plain_form(gpu_session)


def test_older_counting_bits_on_a_mixed_build(gpu_session):
    C.case_counting_bits(gpu_session)


def test_realistic_mix(gpu_session):
    """synth.config3(0.1), two event types: every row against the oracle, on against off bit for bit, and rows of the body from both lists in both event types
    (the test cannot pass with the path dead), no more of them than their classes hold."""
    from universal_recommender_amd import synth
    cfg = synth.config3(0.1)
    data = synth.generate(cfg)[:2]
    mats = [O.Csr(cfg.n_users, nc, rp, ci.astype(np.int32)) for (_, nc, rp, ci) in data]
    params = [O.DatasetParams(500, 50, None) for _ in mats]
    bins = C.check(gpu_session, mats, params, seed=1)
    got = C.body_rows(gpu_session, mats, params, 1)
    print(f"rows by class {[b.tolist() for b in bins]}; rows of the body, of its fallback, per list and event type {got}")
    assert all(0 < g[0][0] <= b[1] and 0 < g[1][0] <= b[2] for g, b in zip(got, bins)), (got, bins)


TIMEOUT = 90          # seconds: two builds of 1,000,000 item rows, each against the oracle and five more times (as the child of test_gpu_small_wave.py)
FAULT_CODES = (124, 134, 137, 139)


def test_production_default_in_a_child_process():
    """The library's own threshold: a catalogue of 1,000,000 item rows, mostly empty, splits the classes; one of 999,999 keeps one list each."""
    torch.cuda.empty_cache()
    env = {k: v for k, v in os.environ.items() if k not in ("URCCO_MICRO_SPLIT_ROWS", C.LIST_ENV)}
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "block_small_wave_child.py")], env=env, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired as e:
        out = (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        err = (e.stderr or b"").decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.exit(f"block_small_wave_child.py ran into its {TIMEOUT} s limit; the GPU may be hung, no further test is started\n{out[-3000:]}\n{err[-3000:]}", returncode=3)
    tail = r.stdout[-6000:] + "\n" + r.stderr[-4000:]
    if r.returncode < 0 or r.returncode in FAULT_CODES:
        pytest.exit(f"block_small_wave_child.py died with status {r.returncode}; the GPU may be faulted, no further test is started\n{tail}", returncode=3)
    assert r.returncode == 0, tail
    assert r.stdout.rstrip().splitlines()[-1] == "BLOCK_SMALL_WAVE_OK", tail
    print(r.stdout)
    builds = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [b["item_rows"] for b in builds] == [1_000_000, 999_999], builds
    assert all(rows > 0 and fb > 0 for rows, fb in builds[0]["body_rows"][1]), builds
    assert all(rows == 0 and fb == 0 for ev in builds[1]["body_rows"] for rows, fb in ev), builds
