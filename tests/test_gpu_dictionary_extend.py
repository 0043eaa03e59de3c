"""The growable device dictionary on hardware: the cases of tests/dictionary_extend_cases.py, each run twice with identical results; the cases that live
on contention -- 64 new keys of one wave on one empty slot, one key 100 000 times in a batch -- run five times and want five identical tables of ids (the
CAS and the stale-read shortcuts of dx_insert_kernel only exist here).  And one stream of production shape: 2^20 + 77 keys, Zipf(1.2) over 2^18 distinct
keys, in five uneven batches against one build."""
import numpy as np
import pytest
import torch

import dictionary_extend_cases as X
from universal_recommender_amd import ingest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_batches", [1, 2, 7])
def test_one_stream_in_batches(gpu_session, n_batches):
    X.case_batching(gpu_session, n_batches, repeat=2)


def test_growth_on_the_capacity_rule(gpu_session):
    X.case_growth(gpu_session, repeat=2)


def test_chain_that_wraps_is_rehashed(gpu_session):
    X.case_chain_wraps_then_rehash(gpu_session, repeat=2)


def test_new_keys_in_old_chains(gpu_session):
    X.case_new_keys_in_old_chains(gpu_session, repeat=2)


@pytest.mark.parametrize("base", [0, X.D.SCAN_TILE - 32])
def test_one_wave_one_slot(gpu_session, base):
    X.case_one_wave_one_slot(gpu_session, base, repeat=5)


def test_one_key_a_hundred_thousand_times(gpu_session):
    X.case_hot_key(gpu_session, repeat=5)


def test_first_appearances_on_tile_edges(gpu_session):
    X.case_tile_edges(gpu_session, repeat=2)


def test_select(gpu_session):
    X.case_select(gpu_session, repeat=2)


def test_extreme_keys(gpu_session):
    X.case_extreme_keys(gpu_session, repeat=2)


@pytest.mark.parametrize("grows", [False, True])
def test_refusals_leave_the_table_as_it_was(gpu_session, grows):
    X.case_refusals(gpu_session, grows, repeat=2)


def test_table_of_min_count_2_is_refused(gpu_session):
    X.case_min_count_table_is_refused(gpu_session)


def test_collisions_are_counted_and_raised(gpu_session):
    X.case_collisions(gpu_session, repeat=2)


def test_ids_may_be_null_and_batches_empty(gpu_session):
    X.case_nullable_ids_and_empty_batches(gpu_session)


def test_zipf_stream_in_five_uneven_batches_against_one_build(gpu_session):
    """numpy holds the restatement here (a Python dict over a million positions would be the slow part): np.unique's first indices, ranked, are the ids."""
    sess = gpu_session
    n, distinct = 2 ** 20 + 77, 2 ** 18
    rng = np.random.default_rng(1202)
    who = np.minimum(rng.zipf(1.2, n) - 1, distinct - 1)
    who[who == distinct - 1] = rng.integers(0, distinct, int((who == distinct - 1).sum()))      # the clipped tail spread over the whole pool
    pool = rng.permutation(np.arange(1, distinct + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))      # distinct (an odd multiplier), never ~0
    keys = pool[who]
    uniq, first = np.unique(keys, return_index=True)
    order = np.argsort(first)
    want_first = first[order].astype(np.int64)
    rank = np.empty(order.size, np.int32)
    rank[order] = np.arange(order.size, dtype=np.int32)
    want_ids = rank[np.searchsorted(uniq, keys)]
    dk = torch.from_numpy(keys.view(np.int64)).to(sess.device)
    cuts = [0, 1, 2 ** 18 + 3, 2 ** 18 + 2051, 2 ** 19 + 2 ** 18, n]      # batches of 1, 2^18 + 2, 2048, about 2^19 and the rest
    d = ingest.dictionary_build(sess, dk[:0])
    one = ingest.dictionary_build(sess, dk)
    try:
        firsts = []
        for a, b in zip(cuts, cuts[1:]):
            ids, new_pos = d.extend(dk[a:b])
            assert X.D.same(ids, want_ids[a:b]), (a, b)
            firsts.append(new_pos.cpu().numpy() + a)
        assert d.n_ids == one.n_ids == uniq.size
        assert np.array_equal(np.concatenate(firsts), want_first) and X.D.same(one.first_pos, want_first)
        assert X.D.same(ingest.dictionary_lookup(sess, d, dk), want_ids) and X.D.same(ingest.dictionary_lookup(sess, one, dk), want_ids)
    finally:
        d.close()
        one.close()
