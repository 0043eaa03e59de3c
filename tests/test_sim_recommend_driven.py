"""The driven class of urcco_dev_recommend_driven (URCCO_REC_DRIVEN, decision D32) on the host simulator (kernel LOGIC on the CPU): every case of
tests/recommend_driven_cases.py, and the argument checks of the entry point."""
import pytest

import recommend_driven_cases as D
from universal_recommender_amd import _lib


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: "-".join(map(str, c)))
def test_driven_class(sim_session, monkeypatch, case):
    getattr(D, case[0])(D.H.Context(sim_session, monkeypatch), *case[1:])


BAD = {
    "rule_beyond": lambda any_, none, cp, ri, rows: dict(rules=[any_], drivers=[(1, cp, ri)], clause_rows=rows),
    "rule_negative": lambda any_, none, cp, ri, rows: dict(rules=[any_], drivers=[(-1, cp, ri)], clause_rows=rows),
    "rule_not_any": lambda any_, none, cp, ri, rows: dict(rules=[any_, none], drivers=[(1, cp, ri)], clause_rows=rows),
    "rule_twice": lambda any_, none, cp, ri, rows: dict(rules=[any_], drivers=[(0, cp, ri), (0, cp, ri)], clause_rows=rows),
    "too_many": lambda any_, none, cp, ri, rows: dict(rules=[any_], drivers=[(0, cp, ri)] * (_lib.REC_MAX_RULES + 1), clause_rows=rows),
    "half_driver": lambda any_, none, cp, ri, rows: dict(rules=[any_], drivers=[(0, cp, None)], clause_rows=rows),
    "half_rows": lambda any_, none, cp, ri, rows: dict(rules=[any_], drivers=[(0, cp, ri)], clause_rows=[(rows[0][0], None)] + rows[1:]),
    "no_rows": lambda any_, none, cp, ri, rows: dict(rules=[any_], drivers=[(0, cp, ri)], clause_rows=None),
    "flag_plain": lambda any_, none, cp, ri, rows: dict(),
    "flag_rules": lambda any_, none, cp, ri, rows: dict(rules=[any_]),
    "flag_weighted": lambda any_, none, cp, ri, rows: dict(rules=[any_], weights=[None] * len(rows)),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_bad_arguments(sim_session, what):
    dp, dr, rules = D.mixed_setup(sim_session)
    rows = [(D.R._dev(sim_session, cl.ind_rp), D.R._dev(sim_session, cl.ind_ci)) for cl in dp.p.clauses]
    kw = BAD[what](dr.dev["any"], dr.dev["none"], *D.csc(sim_session, rules[0]), rows)
    with pytest.raises(_lib.UrccoError) as e:
        sim_session.recommend(dp.n_queries, dp.p.n_items, dp.clauses, 20, flags=D.DRIVEN, **kw)
    assert e.value.status == _lib.BAD_ARG
