"""The premise of tests/golden/landing_cases.json, on the CPU: the oracle still converges each (cheap) case at the iteration the fixture
names, every residual of the solve lies at least 1e-9 (relative) away from eps -- no summation order can move the converged iteration --
and the host-loop restatement of make_landing_cases.py gives the counters the fixture lists."""
import json
import os
import sys

import pytest

from oracle import cz_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
with open(os.path.join(HERE, "golden", "landing_cases.json")) as _f:
    FIX = json.load(_f)
CHEAP = [c for c in FIX["cases"] if c["name"] in ("jacobi_pair_sweep1_poll_first", "jacobi_triple_sweep2_poll_last", "sor2sma_rb4_iter1_poll_last",
                                                  "sor2sma_rb4_itrmax_short", "jacobi_triple_itrmax_short", "pcr_rb", "jacobi_maf_sweep1")]


def test_fixture_is_complete():
    names = {c["name"] for c in FIX["cases"]}
    assert len(CHEAP) == 7 and FIX["eps"] == O.EPS and FIX["margin"] >= 1e-9
    for want in ("jacobi_single_", "jacobi_pair_sweep1", "jacobi_pair_sweep2", "jacobi_triple_sweep1", "jacobi_triple_sweep2", "jacobi_triple_sweep3",
                 "sor2sma_one", "sor2sma_rb4_iter1", "sor2sma_rb4_iter2", "jacobi_maf", "sor2sma_maf", "psor", "pcr_rb", "_itrmax_equal",
                 "_itrmax_short", "decomposed_2x1x1_lag0", "decomposed_2x1x1_lag1", "decomposed_1x2x2_lag0", "decomposed_1x2x2_lag1"):
        assert any(want in n for n in names), want
    for c in FIX["cases"]:
        assert c["counters"], c["name"]


@pytest.mark.parametrize("c", CHEAP, ids=[c["name"] for c in CHEAP])
def test_landing_premise_on_the_oracle(c):
    import make_landing_cases as M
    o = O.run(c["gsz"], c["solver"], c["itr_max"], c["coef"], None, kind="oracle", prec=c["prec"], wide=True)
    assert o.itr == c["iter"]
    assert all(abs(r - O.EPS) >= 1e-9 * O.EPS for _, r in o.history)
    it, cnt = M.counters(c["solver"], c["mode"], c["converged_at"], c["itr_max"])
    assert it == c["iter"] and cnt == c["counters"]


def test_generator_reproduces_the_fixture(tmp_path, monkeypatch):
    """make_landing_cases.py is deterministic: a fresh run writes the committed file byte for byte."""
    import make_landing_cases as M
    monkeypatch.setattr(M, "OUT", str(tmp_path / "landing_cases.json"))
    M.main()
    with open(M.OUT, "rb") as a, open(os.path.join(HERE, "golden", "landing_cases.json"), "rb") as b:
        assert a.read() == b.read()
