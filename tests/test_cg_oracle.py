"""PCG on the CPU: the oracle's restatement (tests/cg_parity.py) against an independent CG, the symmetry and definiteness of the Jacobi(8)
preconditioner that PCG accepts, the premise of the GPU parity cases, and the `cz` command line's usage text."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cg_parity as CP  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not O.have("oracle", "f64"), reason="oracle library not built (make -C oracle)")


def _inner(cz):
    g, (ist, ied, jst, jed, kst, ked) = O.GUIDE - 1, cz.idx
    return (slice(jst + g, jed + g + 1), slice(ist + g, ied + g + 1), slice(kst + g, ked + g + 1))


def _apply_a(u, inner):
    """the 7-point operator ss - 6 u on the inner box of a padded array whose other cells are the Dirichlet data / zero"""
    out = np.zeros_like(u)
    j, i, k = inner
    c = u[j, i, k]
    ss = (u[j, i.start + 1:i.stop + 1, k] + u[j, i.start - 1:i.stop - 1, k] + u[j.start + 1:j.stop + 1, i, k] + u[j.start - 1:j.stop - 1, i, k]
          + u[j, i, k.start + 1:k.stop + 1] + u[j, i, k.start - 1:k.stop - 1])
    out[inner] = ss - 6.0 * c
    return out


def test_pcg_restatement_matches_numpy_cg():
    """(a) the oracle loop with no preconditioner, FP64, against a textbook float64 CG on the same matrix: 10 iterations, 1e-12 relative."""
    gsz = (13, 11, 17)
    r = CP.run(gsz, 10, 0.8, "none", prec="f64", dots="exact")
    cz = CP.CZ(O.Kernels("oracle", "f64"))
    cz.setup(gsz, 0.8)
    inner = _inner(cz)
    x = cz.P.copy()
    res = cz.RHS - _apply_a(x, inner)  # r = b - A x on the inner box (the faces of x are the Dirichlet data)
    rr = np.zeros_like(x)
    rr[inner] = res[inner]
    p = rr.copy()
    rho = float(np.vdot(rr[inner], rr[inner]))
    hist = []
    for _ in range(10):
        q = _apply_a(p, inner)
        alpha = rho / float(np.vdot(p[inner], q[inner]))
        x[inner] += alpha * p[inner]
        rr[inner] -= alpha * q[inner]
        rho_new = float(np.vdot(rr[inner], rr[inner]))
        hist.append(np.sqrt(rho_new * cz.res_normal))
        p[inner] = rr[inner] + (rho_new / rho) * p[inner]
        rho = rho_new
    assert r.itr == 10 and len(r.history) == 10
    scale = np.abs(x[inner]).max()
    assert np.abs(r.P[inner] - x[inner]).max() <= 1e-12 * scale
    np.testing.assert_allclose([h for _, h in r.history], hist, rtol=1e-12)
    assert hist[-1] < 0.5 * hist[0]  # it does converge


@pytest.mark.parametrize("omega", [0.8, 1.0])
def test_jacobi8_preconditioner_is_symmetric_and_definite(omega):
    """(b) M^-1 = 8 relaxed Jacobi sweeps from zero (what PCG's `jacobi` runs) is a symmetric matrix, definite with A's sign, for 0 < omega <= 1"""
    gsz = (7, 6, 8)
    cz = CP.CZ(O.Kernels("oracle", "f64"))
    cz.setup(gsz, omega)
    inner = _inner(cz)
    k = cz.k

    def minv(v):
        b = k.alloc(cz.size)
        b[inner] = v.reshape(b[inner].shape)
        z = k.alloc(cz.size)
        cz.Preconditioner(z, b, "jacobi")
        return z[inner].ravel().copy()

    n = cz.RHS[inner].size
    rng = np.random.default_rng(7)
    u, v = rng.standard_normal(n), rng.standard_normal(n)
    a, b = float(u @ minv(v)), float(v @ minv(u))
    assert abs(a - b) <= 1e-13 * (abs(a) + abs(b))
    M = np.stack([minv(e) for e in np.eye(n)], axis=1)
    assert np.abs(M - M.T).max() <= 1e-14 * np.abs(M).max()
    ev = np.linalg.eigvalsh(0.5 * (M + M.T))
    assert ev.max() < 0.0, ev.max()  # A = ss - 6 I is negative definite, and so is M^-1


@pytest.mark.parametrize("c", CP.CASES + CP.DECOMP_CASES, ids=lambda c: c["id"])
def test_pcg_parity_premise(c):
    """(c) the premise of tests/test_gpu_pcg.py on the oracle alone: FP32 -- no dot of the K iterations lies within its summation bound of a float
    rounding boundary, and the runs with every dot at an edge of its bound are bit-identical; FP64 -- the envelope stays below 1e-8 relative at
    every compared iteration count.  A failure means: choose another case."""
    if c["prec"] == "f32":
        r = CP.premise_f32(c)
    else:
        for kk in CP.ks(c):
            r, _, _ = CP.envelope_f64(c, kk)
    assert len(r.history) == c["K"] >= 3  # not converged before K: every iteration compared is a full one


def test_cli_usage_lists_pcg():
    """(d) the `cz` command line's usage text (printed before any GPU call) names the solver and its preconditioners"""
    exe = os.path.join(ROOT, "cubez_amd", "cz_f32")
    assert os.path.exists(exe), "build() makes cubez_amd/cz_f32"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout
    solvers = out.split("linear_solver = {", 1)[1].split("}", 1)[0]
    assert "pcg" in [s.strip() for s in solvers.split("|")], out
    assert "pcg: none | jacobi" in out and "pcg 1000 0.8 jacobi" in out, out
