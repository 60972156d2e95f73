"""Exact starts and scaled problems on the restatements of pcg (CPU): the contract tests/test_gpu_exact_start.py asks of the
GPU driver -- a solve whose initial residual is exactly zero returns itr = 0 with the field bit-identical to its start -- holds on every
restatement, and the scaling facts that test relies on (K iterations of (p, b) * 2^-s scale bit for bit; the first s that stops) are
measured here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_start as X  # noqa: E402
import problem_parity as PP  # noqa: E402
import project_parity as J  # noqa: E402


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("name", list(X.STATES))
@pytest.mark.parametrize("gsz", X.BOXES, ids=["x".join(map(str, g)) for g in X.BOXES])
def test_the_start_is_exact(gsz, name, kind):
    """b - (sum of the six neighbours - 6 p) == 0 at every inner cell, p's face layers are those the state keeps, and FP32 holds the same
    values as FP64"""
    state = X.STATES[name]
    b, p = X.start(gsz, "f64", state, kind)
    assert np.array_equal(J.fill_field(p, state), p)
    assert not (b[1:-1, 1:-1, 1:-1] - J.laplace(p)).any()
    b32, p32 = X.start(gsz, "f32", state, kind)
    assert np.array_equal(b32.astype(np.float64), b) and np.array_equal(p32.astype(np.float64), p)
    if kind == "integers":
        assert p[1:-1, 1:-1, 1:-1].any() and b.any()
        if state[2]:
            assert float(p[1:-1, 1:-1, 1:-1].sum()) == 0.0


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("pc", X.PCS)
@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("name", list(X.STATES))
def test_restatements_stop_before_they_touch_the_field(name, kind, pc, prec):
    """itr = 0, res = 0, no history, and the field bit-identical to the start, on both boxes"""
    for gsz in X.BOXES:
        b, p = X.start(gsz, prec, X.STATES[name], kind)
        o = X.restated(gsz, pc, prec, name, b, p)
        what = (gsz, name, kind, pc, prec)
        assert o.itr == 0 and o.res == 0.0 and not o.history, (what, o.itr, o.res)
        assert PP.unpad(o.P).tobytes() == p.tobytes(), what


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_discrete_curl_is_divergence_free(prec):
    for gsz in X.BOXES:
        vel = X.divergence_free(gsz, prec)
        assert all(v.any() for v in vel)
        b, ss = J.div(vel, (0, 0, 0), 1.0, X.real(prec))
        assert ss == 0.0 and not b.any()


def _run(prec, pc, s, itr_max):
    b, p = X.scaled_problem(prec, s)
    return X.restated(X.SCALE_BOX, pc, prec, "dirichlet", b, p, itr_max=itr_max, eps=X.EPS_BELOW_REACH)


@pytest.mark.parametrize("prec,pc", list(X.SCALED), ids=[f"{q}_{pc}" for q, pc in X.SCALED])
def test_k_iterations_scale_bit_for_bit_on_the_restatement(prec, pc):
    """the exact-dot restatement (no summation order: the same bits in every run): field and history of (p, b) * 2^-s are those of (p, b)
    times 2^-s, K = 5 iterations"""
    o0 = _run(prec, pc, 0, X.SCALE_K)
    assert o0.itr == X.SCALE_K and len(o0.history) == X.SCALE_K
    for s in X.SCALED[prec, pc]:
        f = 2.0 ** -s
        o = _run(prec, pc, s, X.SCALE_K)
        assert o.itr == X.SCALE_K, (prec, pc, s, o.itr)
        assert o.P.tobytes() == (o0.P * o0.P.dtype.type(f)).tobytes(), (prec, pc, s)
        assert [v for _, v in o.history] == [v * f for _, v in o0.history], (prec, pc, s)


@pytest.mark.parametrize("prec,pc", list(X.FIRST_STOP), ids=[f"{q}_{pc}" for q, pc in X.FIRST_STOP])
def test_the_first_shift_that_stops(prec, pc):
    """rho scales by 4^-s against the absolute FLT_MIN: below FIRST_STOP the first iteration runs, from it on the solve stops with the field
    untouched (one iteration is enough to tell)"""
    first = X.FIRST_STOP[prec, pc]
    found = next(s for s in range(first - 6, first + 7) if _run(prec, pc, s, 1).itr == 0)
    print(f"{prec} {pc}: the first s that stops is {found}")
    assert found == first
    assert X.STOPS.get((prec, pc), first) >= first
    for s in sorted({first, first + 1, X.STOPS.get((prec, pc), first)}):
        o = _run(prec, pc, s, 3)
        assert o.itr == 0 and not o.history and PP.unpad(o.P).tobytes() == X.scaled_problem(prec, s)[1].tobytes(), (prec, pc, s)
