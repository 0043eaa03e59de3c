"""urcco_dev_history_append on the host simulator (kernel LOGIC on the CPU) against the contract of include/urcco.h restated in numpy
(tests/history_append_cases.py): the index of a stream that grew by a batch is the old segments verbatim with the batch's positions behind them, and
the rows over it are the rows over the index built from scratch.  Every output buffer has exactly the size the header names, so the rerun under
HIPSIM_GUARD faults on a write past out_pos[n_old + n_new] or out_row_ptr[n_users + 1]."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import history_append_cases as A
import history_ref as H
from universal_recommender_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def problem():
    return H.make_problem()


@pytest.fixture(scope="module")
def edge():
    return A.make_edge_problem()


def test_index_after_appends(sim_session, problem):
    A.index_cases(sim_session, problem)


def test_edge_problem_holds_the_edge_cases(edge):
    assert A.HA_TILE % 256 == 0
    A.assert_edge_cases(edge)


def test_copy_kernel_edges(sim_session, edge):
    A.edge_case(sim_session, edge)


def test_nothing_written_behind_the_outputs(sim_session, edge):
    A.edge_case(sim_session, edge, pad=64)


def test_id_space_grows_without_events(sim_session, edge):
    """n_new == 0 with n_users > n_users_old: the old index with its last row start repeated"""
    s = sim_session
    rp, pos = s.history_index(A.put(s, edge.old_users), edge.n_users_old)
    new_rp, new_pos = s.history_append(rp, pos, edge.old_users.size, s.empty(0, torch.int32), edge.n_users_old + 3)
    s.synchronize()
    h_rp = rp.cpu().numpy()
    assert np.array_equal(new_rp.cpu().numpy(), np.concatenate([h_rp, [h_rp[-1]] * 3]))
    assert np.array_equal(new_pos.cpu().numpy()[: h_rp[-1]], pos.cpu().numpy()[: h_rp[-1]])


def test_rows_over_an_appended_index(sim_session):
    p, cuts = A.make_rows_problem()
    A.rows_case(sim_session, p, cuts)


def test_bad_arguments(sim_session, edge):
    s = sim_session
    lib = s.lib
    rp, pos = s.history_index(A.put(s, edge.old_users), edge.n_users_old)
    n_old, n_new, nu_old, nu = edge.old_users.size, edge.new_users.size, edge.n_users_old, edge.n_users
    new = A.put(s, edge.new_users)
    out_rp, out_pos = s.empty(nu + 1, torch.int64), s.empty(n_old + n_new, torch.int32)
    ok = dict(s=s.handle, n_old=n_old, nu_old=nu_old, rp=rp.data_ptr(), pos=pos.data_ptr(), n_new=n_new, new=new.data_ptr(), nu=nu, out_rp=out_rp.data_ptr(),
              out_pos=out_pos.data_ptr())

    def call(**kw):
        a = dict(ok, **kw)
        return lib.urcco_dev_history_append(a["s"], a["n_old"], a["nu_old"], a["rp"], a["pos"], a["n_new"], a["new"], a["nu"], a["out_rp"], a["out_pos"])

    assert call() == _lib.OK
    assert call(n_old=(1 << 31) - n_new) == _lib.BAD_ARG                     # n_old + n_new == 2^31
    assert call(n_old=1 << 31, n_new=0) == _lib.BAD_ARG
    assert call(n_old=0, n_new=1 << 31) == _lib.BAD_ARG
    assert call(n_old=(1 << 62), n_new=(1 << 62)) == _lib.BAD_ARG
    assert call(nu=nu_old - 1) == _lib.BAD_ARG                               # a shrinking id space
    for name in ("n_old", "n_new", "nu_old", "nu"):                          # a negative count
        assert call(**{name: -1}) == _lib.BAD_ARG, name
    for name in ("s", "rp", "pos", "new", "out_rp", "out_pos"):              # a NULL the call needs
        assert call(**{name: None}) == _lib.BAD_ARG, name
    # NULLs the call does not need: no old index at all; no batch; an old stream of nobody's events
    assert call(n_old=0, nu_old=0, rp=None, pos=None) == _lib.OK
    assert call(n_new=0, new=None) == _lib.OK
    assert call(nu_old=0, rp=None, pos=None) == _lib.OK
    assert call(n_old=0, nu_old=0, rp=None, pos=None, n_new=0, new=None, nu=0, out_pos=None) == _lib.OK
    s.synchronize()
    assert int(out_rp[0]) == 0                                               # no users: the one row start
    assert lib.urcco_version() == 305


def test_under_guard_pages():
    """This module once more with every buffer ending at a PROT_NONE page (tests/test_sim_guard.py describes the instrument)."""
    if os.environ.get("HIPSIM_GUARD"):
        return  # this IS the guarded run
    env = dict(os.environ, HIPSIM_GUARD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
