"""Mixed-precision refinement restated on the CPU (importable without a GPU): cz_get_residual, cz_add_field and cubez_amd.refine.Refined's loop,
built on the oracle's blas_calc_rk_ and, for the inner solve, on the oracle's FP32 pcg ... mgrb (tests/problem_parity.py, tests/mgrb_parity.py).
tests/test_refine_oracle.py checks it on the CPU, tests/test_gpu_refine.py compares the GPU with it.

Bricks are indexed [i, j, k] (tests/problem_parity.py); the padded arrays of the oracle are [j + 2, i + 2, k + 2].
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import problem_parity as PP  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

CF = (1, 1, 1, 1, 1, 1, 6)
U53 = 2.0 ** -52


def real(prec):
    return np.float32 if prec == "f32" else np.float64


def residual(p, b, prec, nID=(-1,) * 6):
    """r = b - (ss - 6 p) of the brick p, b [i, j, k] in the handle's precision by the oracle's blas_calc_rk_: r on the cells every sweep updates,
    0 on the physical faces (the brick [i, j, k], REAL)"""
    R = real(prec)
    k = PP.Kernels("oracle", prec)
    sz = list(p.shape)
    idx, _ = O.range_inner_index(sz, list(nID))
    r = k.alloc(sz)
    k.blas_calc_rk(r, PP.pad(p.astype(R)), PP.pad(b.astype(R)), sz, idx, np.array(CF, dtype=R))
    return PP.unpad(r)  # (alloc gives zeros: the faces stay 0)


def scaled(r, scale, dtype):
    """what cz_get_residual writes: one multiplication in the handle's precision, then one conversion"""
    return (r * r.dtype.type(scale)).astype(dtype)


def sumsq(r):
    """the correctly rounded sum of the double squares"""
    return math.fsum((r.astype(np.float64).ravel() ** 2).tolist())


def sum_bound(n):
    """relative distance of ANY order of double accumulation of n non-negative terms from their exact sum: each of the n - 1 additions errs by at
    most 2^-53 relative and the terms are of one sign, so the sum errs by at most ((1 + 2^-53)^(n-1) - 1) < n 2^-53 relative; the correctly
    rounded sum is another 2^-53 away.  (n + 1) 2^-52 is twice that and more."""
    return (n + 1) * U53


def add(p, e, scale, inner=None):
    """what cz_add_field leaves in P's brick: p + (REAL)e (REAL)scale on the updated cells (default: all but the outer layer), p elsewhere"""
    R = p.dtype.type
    out = p.copy()
    sl = inner if inner is not None else (slice(1, -1),) * 3
    out[sl] = p[sl] + e.astype(p.dtype)[sl] * R(scale)
    return out


def scale_of(ss, npts):
    """2^-floor(log2 rms): an exact power of two from the sum of squares (cubez_amd.refine.scale_of restated)"""
    m, e = math.frexp(math.sqrt(ss / npts))  # rms = m 2^e, 0.5 <= m < 1
    return math.ldexp(1.0, min(max(1 - e, -100), 100))


INNER_EPS = 1.0e-3  # cubez_amd.refine.INNER_EPS
INNER = dict(solver="pcg", itr_max=1000, coef=1.2, pc="mgrb")


def inner_solve(r32, eps):
    """the oracle's FP32 pcg 1000 1.2 mgrb on A e = r32 from a zero field: (e32, iterations)"""
    c = PP.case(r32.shape, INNER["solver"], INNER["coef"], "f32", INNER["itr_max"], pc=INNER["pc"])
    o = PP.run(c, b=r32, p=np.zeros(r32.shape, dtype=np.float32), eps=eps)
    return PP.unpad(o.P), o.itr


def refine(b, p, tol=1e-10, max_outer=20, inner_eps=INNER_EPS):
    """Refined.solve restated: returns (outer steps taken or 0, history [(outer, |r| / |r0|, inner iterations)], p, ratios) -- ratios: every
    |r| / |r0| the loop compared with tol, the first (1.0) included"""
    p = p.astype(np.float64).copy()
    npts = int(np.prod([n - 2 for n in p.shape]))
    ss0 = sumsq(residual(p, b, "f64"))
    ss, hist, ratios, inner, k = ss0, [], [], 0, 0
    while True:
        scale = scale_of(ss, npts)
        r = residual(p, b, "f64")
        ss = sumsq(r)
        rel = math.sqrt(ss) / math.sqrt(ss0)
        ratios.append(rel)
        if k > 0:
            hist.append((k, rel, inner))
        if math.sqrt(ss) <= tol * math.sqrt(ss0):
            return k, hist, p, ratios
        if k == max_outer:
            return 0, hist, p, ratios
        e32, inner = inner_solve(scaled(r, scale, np.float32), inner_eps)
        p = add(p, e32, 1.0 / scale)
        k += 1


def premise(ratios, tol, npts):
    """no compared ratio lies within the summation bound of tol: |r| <= tol |r0| cannot hinge on the order of the two sums (a relative error d of a
    sum of squares is d / 2 of its root; two roots, so the ratio moves by less than 2 (N + 1) 2^-52 relative)"""
    w = 2.0 * sum_bound(npts)
    return all(not (tol * (1.0 - w) <= q <= tol * (1.0 + w)) for q in ratios)


def lambda_min(shape):
    """smallest eigenvalue of the 7-point operator with Dirichlet faces on a box of n_d - 2 unknowns per direction: sum_d 4 sin^2(pi / (2 (m_d + 1)))"""
    return sum(4.0 * math.sin(math.pi / (2.0 * (n - 2 + 1))) ** 2 for n in shape)
