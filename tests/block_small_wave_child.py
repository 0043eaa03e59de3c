"""Helper of tests/test_gpu_block_small_wave.py -- a plain script, not collected by pytest: the small-row body with eight pairs and two users per lane AT THE
LIBRARY'S DEFAULTS on cuda:0.  tests/conftest.py lowers the threshold of the class splits (URCCO_MICRO_SPLIT_ROWS=0) for the whole pytest process; this process
never imports conftest and refuses to start with the variable set.  Rows of block_small_wave_cases (both lists, fast tail and fallback, users up to 128 and
129) as a catalogue of 1,000,000 item rows -- all but a few dozen of them empty --, where the library itself splits the classes, and as one of 999,999, where
each keeps one list: each build against the C oracle, bit for bit against the same build under NO_BLOCK_SMALL_WAVE, and COUNT_BLOCK_SMALL_WAVE against the
numpy model.  One JSON line per build; the last line is BLOCK_SMALL_WAVE_OK."""
import json
import os
import sys

assert "URCCO_MICRO_SPLIT_ROWS" not in os.environ, "this process checks the library's OWN threshold: start it without URCCO_MICRO_SPLIT_ROWS"

try:  # a GPU fault aborts the process: no core dump of a process with GBs mapped (as conftest.py)
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

import block_small_wave_cases as C
from oracle import c_oracle as O
from universal_recommender_amd import _lib

SPLIT_ROWS = 1_000_000


def main():
    from universal_recommender_amd.device import DeviceSession
    assert torch.cuda.is_available(), "needs a HIP device"
    assert os.path.exists(_lib.DEFAULT_PATH), f"{_lib.DEFAULT_PATH} is missing: build the library first (__graft_entry__.build)"
    sess = DeviceSession(torch.device("cuda", 0), _lib.load(_lib.DEFAULT_PATH))
    try:
        k = 50
        specs = [C.spread(w, ca, 40) for w in (100, 400) for ca in (65, 128, 129)] + [C.distinct(w) for w in (256, 257, 290, 291, 512, 513)]
        specs += [C.repeated(w, 64) for w in (257, 512)] + [C.survivors_spec(D, s, k, 5) for D in (280, 480) for s in (59, 60)]
        (a, b), rows = C.build(specs)
        limit_of = C.limit_fn(sess)
        for n_items in (SPLIT_ROWS, SPLIT_ROWS - 1):
            mats = [O.Csr(a.n_rows, n_items, a.row_ptr, a.col_idx), b]
            params = [C.P(k), C.P(k)]
            C.check(sess, mats, params)
            got = C.body_rows(sess, mats, params, 3)
            want = C.model(rows, k, b.n_cols, limit_of, split=n_items >= SPLIT_ROWS)
            # (A'A: every user holds one item, so item t's row is its self pair alone, cA times -- the rows of 65 .. 128 users belong to list 1 there)
            own = C.model([(ca, np.array([ca]), np.array([ca])) for ca, *_ in specs], k, n_items, limit_of, exclude_self=True, split=n_items >= SPLIT_ROWS)
            print(json.dumps({"item_rows": n_items, "body_rows": got, "model": [own, want]}), flush=True)
            assert got[1] == want and got[0] == own, (got, own, want)
            assert want == (((7, 1), (7, 1)) if n_items >= SPLIT_ROWS else ((0, 0), (0, 0))), want
    finally:
        sess.close()
    assert "conftest" not in sys.modules and "URCCO_MICRO_SPLIT_ROWS" not in os.environ
    print("BLOCK_SMALL_WAVE_OK", flush=True)


if __name__ == "__main__":
    main()
