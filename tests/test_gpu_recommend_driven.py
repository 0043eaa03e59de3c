"""The driven class of urcco_dev_recommend_driven (URCCO_REC_DRIVEN, decision D32) on the GPU: every case of tests/recommend_driven_cases.py."""
import pytest

import recommend_driven_cases as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: "-".join(map(str, c)))
def test_driven_class(gpu_session, monkeypatch, case):
    getattr(D, case[0])(D.H.Context(gpu_session, monkeypatch), *case[1:])
