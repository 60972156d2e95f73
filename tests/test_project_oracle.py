"""The projection step on the CPU: the index rules of tests/project_parity.py in exact integer arithmetic, and the
projection end to end on the restatement of the solver, from which the bars of tests/test_gpu_project.py are taken."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_parity as J  # noqa: E402
import problem_parity as PP  # noqa: E402

CASES = [(g, s) for g in J.SMALL for s in J.STATES if J.fits(g, J.STATES[s])]
IDS = ["x".join(map(str, g)) + "_" + s for g, s in CASES]


def _integers(gsz, state):
    vel = J.velocity(gsz, "f64", 1, integers=True)
    p = np.random.default_rng(5).integers(-5, 6, size=gsz).astype(np.float64)
    return vel, J.fill_field(p, state)


@pytest.mark.parametrize("gsz,name", CASES, ids=IDS)
def test_div_of_the_corrected_velocity_is_the_residual_exactly(gsz, name):
    """div(u - grad p) == div u - (sum of neighbours - 6 p) in small integers, p's face layers as the state fills them; FP32 and FP64 agree
    (every value is exact in both); sub_grad writes the elements `written` names and no other"""
    state = J.STATES[name]
    vel, p = _integers(gsz, state)
    new = J.sub_grad(vel, p, state[1], 1.0, np.float64)
    want = J.div_raw(vel, state[1], np.float64) - J.laplace(p)
    assert np.array_equal(J.div_raw(new, state[1], np.float64), want)
    new32 = J.sub_grad([a.astype(np.float32) for a in vel], p.astype(np.float32), state[1], 1.0, np.float32)
    assert np.array_equal(J.div_raw(new32, state[1], np.float32).astype(np.float64), want)
    for a, b, m in zip(vel, new, J.written(gsz, state[1])):
        assert np.array_equal(a[~m], b[~m]) and not m[tuple(-1 if d == 0 else slice(None) for d in range(3))].all()
    for ax in range(3):
        if state[1][ax]:
            f = lambda c: tuple(c if d == ax else slice(1, -1) for d in range(3))  # noqa: E731
            assert np.array_equal(new[ax][f(0)], new[ax][f(gsz[ax] - 2)])


@pytest.mark.parametrize("gsz,name", CASES, ids=IDS)
def test_div_ignores_face_0_of_a_periodic_direction_and_the_last_entry(gsz, name):
    state = J.STATES[name]
    vel, _ = _integers(gsz, state)
    d0 = J.div_raw(vel, state[1], np.float64)
    for ax in range(3):
        vel[ax][tuple(-1 if d == ax else slice(None) for d in range(3))] = 99.0
        if state[1][ax]:
            vel[ax][tuple(0 if d == ax else slice(None) for d in range(3))] = -77.0
    assert np.array_equal(J.div_raw(vel, state[1], np.float64), d0)
    b, ss = J.div(vel, state[1], 3.0, np.float64)
    assert np.array_equal(b[1:-1, 1:-1, 1:-1], 3.0 * d0) and ss == float((d0 * d0).sum())
    inner = np.zeros(gsz, dtype=bool)
    inner[1:-1, 1:-1, 1:-1] = True
    assert not b[~inner].any()


@pytest.mark.parametrize("gsz", J.SMALL, ids=["x".join(map(str, g)) for g in J.SMALL])
def test_closed_box_sum_of_div_is_the_net_boundary_flux(gsz):
    vel = J.velocity(gsz, "f64", 2, integers=True)
    assert float(J.div_raw(vel, (0, 0, 0), np.float64).sum()) == J.boundary_flux(vel)
    walls = J.velocity(gsz, "f64", 2, J.STATES["closed"], integers=True)
    assert J.boundary_flux(walls) == 0.0 and float(J.div_raw(walls, (0, 0, 0), np.float64).sum()) == 0.0
    inflow = J.velocity(gsz, "f64", 2, J.STATES["closed"], integers=True, inflow=3)
    assert float(J.div_raw(inflow, (0, 0, 0), np.float64).sum()) == -3.0 * (gsz[1] - 2) * (gsz[2] - 2)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", list(J.STATES))
def test_projection_end_to_end_on_the_restatement(name, prec):
    """(33, 47, 61), pcg mgrb 1.2, eps 1e-10 (FP32: 1e-5): ||div after||_2 equals ||b - A p||_2 of the returned iterate up to rounding -- the
    two differ by the roundings of the corrected velocity (half an ulp of |u| per face, six faces a cell) and of A p (the six neighbours and
    6 p: a dozen half-ulps of |p|), so their 2-norms differ by at most sqrt(npts) eps (6 max|u| + 12 max|p|); and the ratio to
    ||div before||_2 is the one recorded in project_parity.MEASURED, from which BARS is made"""
    gsz = J.E2E_BOXES[0]
    o = J.e2e(gsz, "mgrb", 1.2, prec, name)
    R = np.float32 if prec == "f32" else np.float64
    npts = np.prod([n - 2 for n in gsz])
    bound = math.sqrt(npts) * float(np.finfo(R).eps) * (6.0 * max(float(np.abs(a).max()) for a in o["vel"]) + 12.0 * float(np.abs(o["p"]).max()))
    after, resid, before = math.sqrt(o["ss1"]), math.sqrt(o["rr"]), math.sqrt(o["ss0"])
    print(f"{name} {prec}: ||div after|| {after:.6e}  ||b - A p|| {resid:.6e}  bound on the difference {bound:.3e}  ratio {after / before:.3e}  itr {o['itr']}")
    assert abs(after - resid) <= bound
    ratio, itr = J.MEASURED[gsz, "mgrb", name, prec]
    assert o["itr"] == itr and after / before == pytest.approx(ratio, rel=2e-3)  # (the table holds four digits)
    assert 0 < o["itr"] < 300 and o["res"] < J.E2E_EPS[prec]
    assert after / before <= J.BARS[name, prec] / 8.0


def test_the_bars_are_many_orders_below_a_lost_face():
    assert set(J.BARS) == {(s, q) for s in J.STATES for q in ("f64", "f32")}
    assert len(J.MEASURED) == len(J.E2E_BOXES) * len(J.E2E_RUNS) * len(J.STATES) * 2
    assert all(v < (1e-9 if q == "f64" else 1e-4) for (s, q), v in J.BARS.items())
    # a lost face: the X- wall of the closed box not corrected (the mirror read as a Dirichlet zero) leaves a ratio of order 1
    gsz, state = (9, 7, 12), J.STATES["closed"]
    vel = J.velocity(gsz, "f64", 0, state)
    _, p = PP.problem(gsz, "f64", 0)
    good = J.sub_grad(vel, J.fill_field(p, state), state[1], 1.0, np.float64)
    bad = J.sub_grad(vel, p, state[1], 1.0, np.float64)
    d = J.div_raw(good, state[1], np.float64) - J.div_raw(bad, state[1], np.float64)
    assert math.sqrt(J.sumsq(d)) > 0.1 * math.sqrt(J.sumsq(J.div_raw(vel, state[1], np.float64)))
