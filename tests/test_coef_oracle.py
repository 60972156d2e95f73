"""Face coefficients for pcg on the CPU: the numpy restatement of tests/coef_parity.py against the oracle and against the
properties the method rests on -- a symmetric negative (semi-)definite operator, a symmetric preconditioner, the exact projection identity,
the faces that are never read -- and the premises of the GPU cases of tests/test_gpu_coef.py."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coef_parity as K  # noqa: E402
import mg_parity as M  # noqa: E402
import periodic_parity as P  # noqa: E402
import problem_parity as PP  # noqa: E402
import project_parity as J  # noqa: E402

SINGULAR = ("closed", "channel", "triple")


def _int_field(gsz, R, seed):
    return np.random.default_rng(4000 + seed).integers(-4, 5, size=tuple(gsz)).astype(R)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", list(K.STATES))
def test_unit_coefficients_are_the_oracles_operator_on_integers(name, prec):
    """beta = 1, small integers: A p and b - A p are the oracle's blas_calc_ax / blas_calc_rk exactly"""
    gsz, state, R = (9, 7, 12), K.STATES[name], K._real(prec)
    sz, idx = K.box(gsz)
    p, b = _int_field(gsz, R, 0), _int_field(gsz, R, 1)
    cf = np.array([1, 1, 1, 1, 1, 1, 6], dtype=R)
    ref, new = P.kernels(prec, state[0], state[1]), K.Kernels("oracle", prec)
    new.faces, new.per, new.B = tuple(state[0]), tuple(state[1]), K.imported(K.ones(gsz, prec), state[1])
    for fn, extra in (("blas_calc_ax", ()), ("blas_calc_rk", (PP.pad(b),))):
        a0, a1 = ref.alloc(sz), new.alloc(sz)
        getattr(ref, fn)(a0, PP.pad(p), *extra, sz, idx, cf)
        getattr(new, fn)(a1, PP.pad(p), *extra, sz, idx, cf)
        assert np.array_equal(a0, a1) and np.abs(a0).max() > 0, fn


@pytest.mark.parametrize("name", list(K.STATES))
def test_assembled_operator_is_symmetric_and_negative(name):
    """(6, 5, 7), integer coefficients 1 .. 4 (exact): A = A^T, no positive eigenvalue; zero row sums exactly in the singular states, and
    there one zero eigenvalue; in the others every eigenvalue is negative"""
    gsz, state = (6, 5, 7), K.STATES[name]
    A = K.assembled(gsz, K.ints(gsz, "f64"), state)
    assert np.array_equal(A, A.T)
    ev = np.linalg.eigvalsh(A)
    rows = A.sum(axis=1)
    if name in SINGULAR:
        assert np.array_equal(rows, np.zeros_like(rows))
        assert abs(ev[-1]) <= 1e-12 * abs(ev[0]) and ev[-2] < -1e-6
    else:
        assert rows.max() <= 0 and rows.min() < 0 and ev[-1] < -1e-6


@pytest.mark.parametrize("pc,coef", [("jacobi", 0.8), ("mg", 0.8), ("mgrb", 1.2)])
@pytest.mark.parametrize("name", ["dirichlet", "inflow"])
def test_scaled_preconditioner_is_symmetric_and_definite(name, pc, coef):
    """s M^-1 s applied to the unit vectors of a tiny box: the matrix is symmetric to rounding and definite with the sign of the operator
    (the stated operator is negative definite, so its approximate inverse is: -M^-1 is the positive definite preconditioner of -A)"""
    gsz, state = (6, 5, 7), K.STATES[name]
    cz, k = K.solver(gsz, coef, "f64", state, K.random(gsz, "f64"))
    cz._mgrb, cz._mg, cz.cycles = pc == "mgrb", pc in ("mg", "mgrb"), 0
    ins = M.inner(cz.size, cz.idx)
    n = [v - 2 for v in gsz]
    N = n[0] * n[1] * n[2]
    Mi = np.zeros((N, N))
    for q in range(N):
        e = np.zeros(tuple(gsz))
        e[1 + q // (n[1] * n[2]), 1 + (q // n[2]) % n[1], 1 + q % n[2]] = 1.0
        z = k.alloc(cz.size)
        cz.Preconditioner(z, PP.pad(e), "jacobi")
        Mi[:, q] = PP.unpad(z)[1:-1, 1:-1, 1:-1].ravel()
        assert not PP.unpad(z)[0].any() and z[ins].any()
    assert np.abs(Mi - Mi.T).max() <= 1e-13 * np.abs(Mi).max()
    assert np.linalg.eigvalsh(0.5 * (Mi + Mi.T))[-1] < 0


IDENTITY = [(g, s) for g in J.SMALL for s in K.STATES if J.fits(g, K.STATES[s])]  # (a periodic direction needs four cells)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz,name", IDENTITY, ids=["x".join(map(str, g)) + "_" + s for g, s in IDENTITY])
def test_projection_identity_is_exact_in_integers(gsz, name, prec):
    """integer velocity, field and coefficients, a power-of-two scale: div(u - beta grad p) == div u - A p, bit for bit"""
    state, R = K.STATES[name], K._real(prec)
    sz, idx = K.box(gsz)
    vel = J.velocity(gsz, prec, 5, integers=True)
    beta = K.ints(gsz, prec)
    p = J.fill_field(_int_field(gsz, R, 2), state)
    scale = 0.25
    new = K.sub_grad(vel, p, beta, state[1], scale, R)
    lhs = J.div_raw(new, state[1], R)
    ap = K.apply(PP.pad(p), K.imported(beta, state[1]), sz, idx).transpose(1, 0, 2)
    rhs = J.div_raw(vel, state[1], R) - R(scale) * ap
    assert np.array_equal(lhs, rhs) and np.abs(ap).max() > 0


@pytest.mark.parametrize("name", ["dirichlet", "px", "triple"])
def test_faces_outside_the_contract_are_never_read(name):
    """NaN on entry n - 1, on face 0 of a periodic direction and on the faces at boundary tangential indices changes nothing: the operator,
    the scaling, the gradient"""
    gsz, state, R = (9, 7, 12), K.STATES[name], np.float64
    sz, idx = K.box(gsz)
    beta = K.random(gsz, "f64")
    bad = [np.where(m, np.nan, b) for b, m in zip(beta, K.unread(gsz, state[1]))]
    assert all(np.isnan(b).any() for b in bad)
    _, p = PP.problem(gsz, "f64", 0)
    pf = J.fill_field(p, state)
    B0, B1 = K.imported(beta, state[1]), K.imported(bad, state[1])
    assert np.array_equal(K.apply(PP.pad(pf), B0, sz, idx), K.apply(PP.pad(pf), B1, sz, idx))
    assert np.array_equal(K.scaling(B0, sz, idx), K.scaling(B1, sz, idx))
    vel = J.velocity(gsz, "f64", 1)
    for a, b in zip(K.sub_grad(vel, pf, beta, state[1], 1.7, R), K.sub_grad(vel, pf, bad, state[1], 1.7, R)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("c", K.PCG_CASES, ids=[c["id"] for c in K.PCG_CASES])
def test_premise_of_the_gpu_pcg_cases(c):
    """FP32: no dot within its summation bound of a rounding boundary (closed states: the sums too), so any summation order gives the
    restatement's bits; FP64: the envelope of the runs with every dot at either edge of its bound stays below 1e-8"""
    b, p, beta = K.case_problem(c)
    state = K.STATES[c["state"]]
    if c["prec"] == "f32":
        r = K.premise_f32(c["gsz"], c["pc"], c["coef"], state, c["K"], b, p, beta, eps=1e-30)
    else:
        r, E, Eh = K.envelope_f64(c["gsz"], c["pc"], c["coef"], state, c["K"], b, p, beta, eps=1e-30)
        print(c["id"], "envelope", float(E.max()), float(Eh.max()))
        assert E.max() <= 1e-8 and Eh.max() <= 1e-8
    assert r.itr == c["K"] and len(r.history) == c["K"]


@pytest.mark.parametrize("pc,coef", K.COUNT_RUNS)
def test_iteration_counts_are_the_recorded_ones(pc, coef):
    """the scaled column of coef_parity.COUNTS and the constant operator, re-measured: 33 x 47 x 61, FP64, Dirichlet, eps 1e-8"""
    g = K.COUNT_BOX
    b, p = PP.problem(g, "f64", 0)
    st = K.STATES["dirichlet"]
    got = {"constant": P.run(list(g), pc, coef, "f64", st, 300, b, p, eps=K.COUNT_EPS).itr}
    for f in ("smooth4", "smooth10", "bubble10", "bubble100", "aniso4"):
        got[f] = K.run(list(g), pc, coef, "f64", st, 300, b, p, K.FIELDS[f](g, "f64"), eps=K.COUNT_EPS).itr
    assert got == {f: K.COUNTS[f, pc][1] for f in got}


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", list(K.STATES))
def test_measured_projection_rows_are_the_recorded_ones(name, prec):
    """the (33, 47, 61) rows of coef_parity.MEASURED: the ratio to the three digits recorded, the count exactly; and the ratio is that of a
    converged solve (below eps over the RMS of the seeded divergence, about 1.41, times the largest coefficient's part in the identity)"""
    g = (33, 47, 61)
    for pc, coef in K.E2E_RUNS:
        for f in K.E2E_FIELDS:
            o = K.project(g, pc, coef, prec, name, f)
            ratio, itr = K.MEASURED[g, pc, f, name, prec]
            assert o["itr"] == itr and math.isclose(o["ratio"], ratio, rel_tol=2e-3), (pc, f, o["itr"], o["ratio"], ratio, itr)
            assert 0 < itr < 300 and o["ratio"] < J.E2E_EPS[prec]
