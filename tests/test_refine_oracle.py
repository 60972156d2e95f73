"""Mixed-precision refinement on the CPU (no GPU): the restatement tests/refine_parity.py -- cz_get_residual, cz_add_field and Refined's loop on the
oracle's blas_calc_rk_ and FP32 pcg ... mgrb -- does what the feature promises, and the premises tests/test_gpu_refine.py relies on hold."""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import problem_parity as PP  # noqa: E402
import refine_parity as RP  # noqa: E402

BOXES = [(33, 47, 61), (64, 64, 64)]
TOL = 1e-10


@functools.lru_cache(maxsize=None)
def _refined(gsz, eps):
    u, b, p = PP.manufactured(gsz)
    return RP.refine(b, p, tol=TOL, inner_eps=eps)


def _npts(gsz):
    return int(np.prod([n - 2 for n in gsz]))


def test_the_restated_entries_on_a_small_box():
    """r is blas_calc_rk_'s on the inner cells and 0 on the faces; scaling by a power of two and widening commute with it; add touches the
    inner cells only and rounds once per operation"""
    b, p = PP.problem((9, 7, 12), "f32", 11)
    r = RP.residual(p, b, "f32")
    want = np.zeros_like(r)
    q = p.astype(np.float32)
    ss = q[2:, 1:-1, 1:-1] + q[:-2, 1:-1, 1:-1] + q[1:-1, 2:, 1:-1] + q[1:-1, :-2, 1:-1] + q[1:-1, 1:-1, 2:] + q[1:-1, 1:-1, :-2]
    want[1:-1, 1:-1, 1:-1] = b[1:-1, 1:-1, 1:-1] - (ss - np.float32(6) * q[1:-1, 1:-1, 1:-1])
    assert r.tobytes() == want.tobytes()
    assert RP.scaled(r, 2.0 ** 9, np.float64).tobytes() == (r.astype(np.float64) * 512.0).tobytes()
    e = np.full(p.shape, 0.1, dtype=np.float64)
    x = RP.add(p, e, 3.0)
    assert x.dtype == np.float32 and np.array_equal(x[0], p[0]) and np.array_equal(x[:, :, -1], p[:, :, -1])
    assert x[4, 3, 5] == np.float32(p[4, 3, 5] + np.float32(np.float32(0.1) * np.float32(3.0)))
    assert abs(RP.sumsq(r) - float(np.sum(r.astype(np.float64) ** 2))) <= RP.sum_bound(r.size) * RP.sumsq(r)


@pytest.mark.parametrize("gsz", BOXES, ids=lambda g: "x".join(map(str, g)))
def test_the_restated_loop_reaches_1e_10_and_one_fp32_solve_does_not(gsz):
    u, b, p = PP.manufactured(gsz)
    k, hist, x, ratios = _refined(gsz, RP.INNER_EPS)
    print(gsz, "outer", k, "history", hist)
    assert 0 < k <= 20 and hist[-1][1] <= TOL and [h[0] for h in hist] == list(range(1, k + 1))
    r0, rx = RP.residual(p, b, "f64"), RP.residual(x, b, "f64")
    assert math.sqrt(RP.sumsq(rx)) <= TOL * math.sqrt(RP.sumsq(r0))  # (read back independently of the loop's own sums)
    # the premise of the feature: the FP32 library alone, however tight its tolerance, stays orders of magnitude above the bar
    c = PP.case(gsz, "pcg", 1.2, "f32", 60, pc="mgrb")
    o = PP.run(c, b=b.astype(np.float32), p=p.astype(np.float32), eps=1e-10)
    rel = math.sqrt(RP.sumsq(RP.residual(PP.unpad(o.P).astype(np.float64), b, "f64")) / RP.sumsq(r0))
    print(gsz, "one FP32 solve:", o.itr, "iterations, true relative residual", rel)
    assert rel > 1e3 * TOL
    # the premise of every GPU case: no ratio the loop compares with tol lies within the summation bound of it
    assert RP.premise(ratios, TOL, _npts(gsz))
    w = 2.0 * RP.sum_bound(_npts(gsz))
    assert not RP.premise([TOL * (1.0 + 0.5 * w)], TOL, _npts(gsz)) and RP.premise([TOL * (1.0 + 2.0 * w)], TOL, _npts(gsz))


def test_the_inner_eps_table_at_64():
    """total inner iterations to 1e-10 at 64^3: 1e-2 and 1e-3 tie at the fewest, 1e-3 in fewer outer steps (each of which
    costs a residual pass, a correction pass and the inner solve's set-up passes): the default"""
    tab = {}
    for eps in (1e-2, 1e-3, 1e-4):
        k, hist, _, ratios = _refined((64, 64, 64), eps)
        assert k > 0 and RP.premise(ratios, TOL, _npts((64, 64, 64)))
        tab[eps] = (k, sum(h[2] for h in hist))
    print("inner_eps -> (outer steps, inner iterations):", tab)
    assert tab == {1e-2: (7, 14), 1e-3: (5, 14), 1e-4: (5, 17)}
    best = min(tab, key=lambda e: (tab[e][1], tab[e][0]))
    from cubez_amd.refine import INNER_EPS, scale_of
    assert best == INNER_EPS == RP.INNER_EPS
    for ss in (1e-30, 3.7e-9, 1.0, 5e11):
        assert scale_of(ss, 1000) == RP.scale_of(ss, 1000)
        rms = math.sqrt(ss / 1000) * scale_of(ss, 1000)
        assert 1.0 <= rms < 2.0 and math.frexp(scale_of(ss, 1000))[0] == 0.5


def test_lambda_min_is_the_smallest_eigenvalue():
    """on a box small enough to build the matrix"""
    n = (5, 6, 4)
    m = [v - 2 for v in n]
    def lap(k):
        return 2.0 * np.eye(k) - np.eye(k, k=1) - np.eye(k, k=-1)
    A = (np.kron(np.kron(lap(m[0]), np.eye(m[1])), np.eye(m[2])) + np.kron(np.kron(np.eye(m[0]), lap(m[1])), np.eye(m[2]))
         + np.kron(np.kron(np.eye(m[0]), np.eye(m[1])), lap(m[2])))
    assert abs(np.linalg.eigvalsh(A)[0] - RP.lambda_min(n)) < 1e-12
