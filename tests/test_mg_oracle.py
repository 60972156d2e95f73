"""The multigrid V-cycle of `pcg ... mg` on the CPU (tests/mg_parity.py): its restatement agrees with the oracle's sweep, it is a symmetric
definite preconditioner, PCG with it converges in the iteration counts DESIGN.md §5.10 states, and the levels have the stated extents."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cg_parity as CP  # noqa: E402
import mg_parity as M  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402


def _box(gsz):
    idx, _ = O.range_inner_index(list(gsz), [-1] * 6)
    return list(gsz), idx, M.n0_of(idx)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_level0_sweep_is_the_oracles_jacobi(prec):
    """the restated sweep at level 0 (weights 1, D = 6) gives the bits of the oracle's jacobi"""
    k = O.Kernels("oracle", prec)
    R = k.real
    sz, idx, n0 = _box((33, 47, 61))
    ins = M.inner(sz, idx)
    rng = np.random.default_rng(3)
    u, b = k.alloc(sz), k.alloc(sz)
    u[ins], b[ins] = rng.standard_normal(u[ins].shape).astype(R), rng.standard_normal(b[ins].shape).astype(R)
    ref = u.copy()
    k.jacobi(ref, sz, idx, np.array([1, 1, 1, 1, 1, 1, 6], dtype=R), R(0.8), b, k.alloc(sz))
    assert M.smooth(u[ins], b[ins], 0, n0, 0.8).tobytes() == ref[ins].tobytes()
    # and the level-0 residual is blas_calc_rk's
    r = k.alloc(sz)
    k.blas_calc_rk(r, u, b, sz, idx, np.array([1, 1, 1, 1, 1, 1, 6], dtype=R))
    assert M.residual(u[ins], b[ins], 0, n0).tobytes() == r[ins].tobytes()


@pytest.mark.parametrize("gsz,dims", [
    ((9, 7, 12), [(7, 5, 10), (4, 3, 5), (2, 2, 3)]),
    ((3, 40, 40), [(1, 38, 38), (1, 19, 19), (1, 10, 10), (1, 5, 5), (1, 3, 3)]),
    ((40, 40, 1100), [(38, 38, 1098), (19, 19, 549), (10, 10, 275), (5, 5, 138), (3, 3, 69), (2, 2, 35), (1, 1, 18), (1, 1, 9), (1, 1, 5),
                      (1, 1, 3)]),
    ((6, 6, 6), [(4, 4, 4)]),
    ((128, 128, 128), [(126,) * 3, (63,) * 3, (32,) * 3, (16,) * 3, (8,) * 3, (4,) * 3]),
])
def test_level_extents(gsz, dims):
    """ceil(n/2) per level down to the first whose largest extent is <= 4; the extents E of every level cover level 0 exactly, only the
    last point of a direction partial, an extent of 1 stays 1"""
    _, _, n0 = _box(gsz)
    got = M.level_dims(n0)
    assert got == dims
    for l, n in enumerate(got):
        for d in range(3):
            e = M.extents(n0[d], l, n[d])
            assert e.sum() == n0[d] and (e[:-1] == 1 << l).all() and 1 <= e[-1] <= 1 << l


def _apply(k, sz, idx, v_inner, omg=0.8):
    r = k.alloc(sz)
    ins = M.inner(sz, idx)
    r[ins] = v_inner
    return M.apply(k, r, sz, idx, omg)[ins]


def test_preconditioner_is_symmetric():
    """(M r1).r2 = r1.(M r2) to 1e-12 relative, FP64"""
    k = O.Kernels("oracle", "f64")
    for gsz in ((33, 47, 61), (9, 7, 12), (40, 40, 100)):
        sz, idx, _ = _box(gsz)
        rng = np.random.default_rng(5)
        shape = (idx[3] - idx[2] + 1, idx[1] - idx[0] + 1, idx[5] - idx[4] + 1)
        r1, r2 = rng.standard_normal(shape), rng.standard_normal(shape)
        a, b = float(np.vdot(_apply(k, sz, idx, r1), r2)), float(np.vdot(r1, _apply(k, sz, idx, r2)))
        assert abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (gsz, a, b)


def _smallest_ritz(gsz, omg, steps=24):
    """Lanczos on M A (A the fine operator) in the A-inner product, with B = -A and -M both definite; the smallest Ritz value"""
    k = O.Kernels("oracle", "f64")
    sz, idx, n0 = _box(gsz)
    shape = (n0[1], n0[0], n0[2])
    B = lambda v: M.residual(v, np.zeros_like(v), 0, n0)  # 6 v - ss: -A  # noqa: E731
    T = lambda v: -_apply(k, sz, idx, B(v), omg)  # M A v  # noqa: E731
    rng = np.random.default_rng(9)
    v = rng.standard_normal(shape)
    V = [v / np.sqrt(np.vdot(v, B(v)))]
    alphas, betas = [], []
    for j in range(steps):
        w = T(V[j])
        Bw = B(w)
        alphas.append(float(np.vdot(Bw, V[j])))
        for q in V:  # full re-orthogonalisation in the B-inner product
            w = w - float(np.vdot(B(q), w)) * q
        beta = float(np.sqrt(max(np.vdot(w, B(w)), 0.0)))
        if beta < 1e-12 or j == steps - 1:
            break
        betas.append(beta)
        V.append(w / beta)
    n = len(alphas)
    Tm = np.diag(alphas) + np.diag(betas[: n - 1], 1) + np.diag(betas[: n - 1], -1)
    return float(np.linalg.eigvalsh(Tm).min())


@pytest.mark.parametrize("gsz", [(34, 34, 34), (33, 47, 61), (40, 40, 1100)])
def test_preconditioned_operator_is_definite(gsz):
    """the smallest Ritz value of M A stays > 0.1 at omega = 0.8"""
    lo = _smallest_ritz(gsz, 0.8)
    assert lo > 0.1, (gsz, lo)


def test_oracle_iteration_counts():
    """PCG with the V-cycle, FP64, exact dots: <= 10 iterations at 64^3, <= 12 at 128^3, where jacobi takes 36 at 128^3"""
    r64 = M.run((64, 64, 64), 1000, 0.8, prec="f64")
    r128 = M.run((128, 128, 128), 1000, 0.8, prec="f64")
    j128 = CP.run((128, 128, 128), 1000, 0.8, "jacobi", prec="f64")
    assert r64.itr <= 10 and r128.itr <= 12, (r64.itr, r128.itr)
    assert j128.itr == 36
    assert r64.res < O.EPS and r128.res < O.EPS


@pytest.mark.parametrize("c", M.CASES, ids=[c["id"] for c in M.CASES])
def test_pcg_mg_parity_premise(c):
    """the GPU cases of tests/test_gpu_mg.py: FP32 no dot within its summation bound of a rounding boundary; FP64 an envelope that says
    something"""
    if c["prec"] == "f32":
        M.premise_f32(c)
        for p in (-1, 1):
            rp = M.oracle(c, c["K"], p)
            r0 = M.oracle(c, c["K"])
            assert rp.itr == r0.itr and rp.history == r0.history and rp.P.tobytes() == r0.P.tobytes(), (c["id"], p)
    else:
        M.envelope_f64(c, c["K"])
