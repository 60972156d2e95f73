"""GPU tests (-m gpu) of the pass protocol of the stationary solvers end to end: every case of tests/golden/landing_cases.json (written by
make_landing_cases.py from the oracle) converges at a chosen position -- the first, second or third iteration of a launch, the launch before
a host poll or after it, ItrMax at or one short of the converged iteration, decomposed SPLIT pairs with and without the lagged reduce.  The
solve through CZ must give the oracle's iteration count and residual, its field bit for bit and its history, and show through info() that it
ran the path the case names (re-runs, triples, rb4 passes, pass kind, buffers)."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import cz_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "landing_cases.json")) as _f:
    CASES = json.load(_f)["cases"]
SINGLE = [c for c in CASES if "div" not in c]
DECOMP = [c for c in CASES if "div" in c]


def _rtol(c):
    return 1e-10 if c["solver"].startswith("pcr") or c["gsz"][0] != c["gsz"][1] or c["gsz"][1] != c["gsz"][2] else 1e-11


def _oracle(c):
    o = O.run(c["gsz"], c["solver"], c["itr_max"], c["coef"], None, kind="oracle", prec=c["prec"], wide=True)
    assert o.itr == c["iter"], (c["name"], o.itr)  # the fixture still describes the oracle
    return o


def _check_run(c, o, itr, res, hist, P, info):
    assert itr == c["iter"], (c["name"], itr, c["iter"])
    assert abs(res - o.res) <= 1e-10 * o.res, (c["name"], res, o.res)
    assert len(hist) == len(o.history), (c["name"], len(hist), len(o.history))
    assert np.allclose(hist, [r for _, r in o.history], rtol=_rtol(c), atol=0), c["name"]
    if P is not None:
        assert P.tobytes() == o.P.tobytes(), f"{c['name']}: field differs from the oracle"
    for k, v in c["counters"].items():
        assert info[k] == v, (c["name"], k, info[k], v, info)


@pytest.mark.parametrize("c", SINGLE, ids=[c["name"] for c in SINGLE])
def test_single_domain_landing(c):
    from cubez_amd import CZ
    sw = c["switches"]
    cz = CZ(c["prec"], quiet=True)
    cz.lib.czhip_set_tuning2(0, 0, -1, sw["t2"])
    cz.lib.czhip_set_jac3(sw["jac3"], -1, -1)
    cz.lib.czhip_set_rb4(sw["rb4"], -1, -1)
    try:
        assert cz.setup(list(c["gsz"]) + [c["solver"], c["itr_max"], c["coef"]]) == 1
        itr = cz.solve()
        run = (itr, cz.res, list(cz.history()), cz.field(), cz.info())
    finally:
        cz.lib.czhip_set_tuning2(0, 0, -1, 1)
        cz.lib.czhip_set_jac3(1, -1, -1)
        cz.lib.czhip_set_rb4(1, -1, -1)
        cz.close()
    _check_run(c, _oracle(c), *run)


@pytest.mark.parametrize("c", DECOMP, ids=[c["name"] for c in DECOMP])
def test_decomposed_landing(c):
    """LOCAL transport: every rank reports the oracle's iteration count, residual and history, the assembled field equals the oracle's."""
    from test_gpu_decomp import _decomposed
    o = _oracle(c)
    results, G = _decomposed(c["prec"], c["gsz"], c["solver"], c["itr_max"], c["coef"], tuple(c["div"]),
                             env={"CZ_LAG_REDUCE": str(c["lag_reduce"])})
    inner = (slice(2, -2),) * 3
    for itr, res, hist, P, loc in results:
        _check_run(c, o, itr, res, hist, None, loc["info"])  # (the field: assembled below)
    assert G[inner].tobytes() == o.P[inner].tobytes(), f"{c['name']}: field differs from the oracle"
