"""The hashed accumulator class of urcco_dev_recommend (URCCO_REC_HASHED, decision D31) on the host simulator (kernel LOGIC on the CPU): every case of
tests/recommend_hashed_cases.py."""
import pytest

import recommend_hashed_cases as H


@pytest.mark.parametrize("case", H.CASES, ids=lambda c: "-".join(map(str, c)))
def test_hashed_class(sim_session, monkeypatch, case):
    getattr(H, case[0])(H.Context(sim_session, monkeypatch), *case[1:])
