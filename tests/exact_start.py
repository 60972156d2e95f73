"""Exact starts and scaled problems for pcg (importable without a GPU): what tests/test_exact_start_oracle.py checks on
the restatements and tests/test_gpu_exact_start.py asks of the GPU driver.

An exact start is a pair (b, p) whose initial residual b - A p is zero in every bit, so that rho = r.z = 0 and the solve must stop at
iteration 1 with itr = 0 BEFORE it touches p:
    "zero"      b = 0, p = 0 (a fluid at rest)
    "integers"  p small integers in -8 .. 8 with the face layers the state keeps (wrap, mirror), b = sum of the six neighbours - 6 p computed
                in integers: every operation of the residual is exact in FP32 and FP64, whatever its order.  In the closed box the inner
                cells of p sum to zero, so the projection of the answer subtracts an exact 0; b then sums to zero by itself.

A scaled problem is (b, p) * 2^-s: every operation of a pcg iteration commutes with a power of two until something underflows, so the field
and the history scale exactly -- until rho = r.z (which scales by 4^-s) falls under the ABSOLUTE threshold FLT_MIN = 2^-126 of both
precisions and the solve stops at iteration 1.  FIRST_STOP records, per (precision, preconditioner), the first s at which the restatement
stops at 33x47x61 on the built-in test case (tests/test_exact_start_oracle.py re-measures it).
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_parity as C  # noqa: E402
import neumann_parity as N  # noqa: E402
import periodic_parity as P  # noqa: E402
import problem_parity as PP  # noqa: E402
import project_parity as J  # noqa: E402

BOXES = [(9, 7, 12), (33, 47, 61)]
PCS = ["none", "jacobi", "mg", "mgrb"]
COEF = 0.8
# (Neumann faces, periodic directions, closed)
STATES = {"dirichlet": (N.NONE, P.NOPER, False), "neumann_z": (N.Z_BOTH, P.NOPER, False), "periodic_xz": (N.NONE, P.PXZ, False),
          "closed": (C.SIX, P.NOPER, True)}
KINDS = ["zero", "integers"]


def real(prec):
    return np.float32 if prec == "f32" else np.float64


def start(gsz, prec, state, kind, seed=0):
    """(b, p) [i, j, k] of an exact start under `state`; p carries the face layers the handle keeps, so get_field returns its bytes"""
    R = real(prec)
    if kind == "zero":
        return np.zeros(gsz, dtype=R), np.zeros(gsz, dtype=R)
    rng = np.random.default_rng(3000 + seed)
    p = rng.integers(-7, 8, size=tuple(gsz)).astype(np.int64)
    if state[2]:  # zero sum over the inner cells: the excess goes, one unit a cell, to the first cells (|p| stays <= 8)
        inner = p[1:-1, 1:-1, 1:-1]
        s = int(inner.sum())
        flat = inner.reshape(-1)  # (a copy: the slice is not contiguous)
        assert abs(s) <= flat.size
        flat[:abs(s)] -= np.sign(s)
        p[1:-1, 1:-1, 1:-1] = flat.reshape(inner.shape)
        assert int(p[1:-1, 1:-1, 1:-1].sum()) == 0
    pf = J.fill_field(p.astype(np.float64), state)
    b = np.zeros(gsz, dtype=np.float64)
    b[1:-1, 1:-1, 1:-1] = J.laplace(pf)
    assert np.abs(pf).max() <= 8 and np.abs(b).max() <= 96 and (not state[2] or float(b.sum()) == 0.0)
    return b.astype(R), pf.astype(R)


def divergence_free(gsz, prec, seed=0):
    """an integer staggered velocity (u, v, w) [i, j, k] whose discrete divergence (project_parity.div_raw, no periodic direction) is exactly
    zero at every inner cell: the discrete curl of an integer vector potential (a, b, c) on the cell edges,
        u = (c(j) - c(j-1)) - (b(k) - b(k-1)),  v = (a(k) - a(k-1)) - (c(i) - c(i-1)),  w = (b(i) - b(i-1)) - (a(j) - a(j-1)),
    whose divergence telescopes to zero term by term; index 0 of a differenced direction holds 0"""
    R = real(prec)
    rng = np.random.default_rng(4000 + seed)
    a, b, c = (rng.integers(-3, 4, size=tuple(gsz)).astype(np.int64) for _ in range(3))

    def d(f, ax):
        out = np.zeros_like(f)
        sl = [slice(None)] * 3
        lo = list(sl)
        sl[ax], lo[ax] = slice(1, None), slice(0, -1)
        out[tuple(sl)] = f[tuple(sl)] - f[tuple(lo)]
        return out

    vel = [d(c, 1) - d(b, 2), d(a, 2) - d(c, 0), d(b, 0) - d(a, 1)]
    return [v.astype(R) for v in vel]


def restated(gsz, pc, prec, name, b, p, itr_max=20, eps=None):
    """`pcg itr_max COEF pc` on (b, p) under STATES[name], on the restatement that owns the state: cg / mg / mgrb_parity through
    problem_parity.run (Dirichlet), neumann_parity.run, periodic_parity.run, closed_parity.run.  O.Result"""
    state = STATES[name]
    if name == "dirichlet":
        c = PP.case(gsz, "pcg", COEF, prec, itr_max, pc=pc, eps=eps)
        return PP.run(c, b=b, p=p)
    if name == "neumann_z":
        return N.run(list(gsz), pc, COEF, prec, state[0], itr_max, b, p, eps=eps)
    if name == "closed":
        return C.run(list(gsz), pc, COEF, prec, itr_max, b, p, eps=eps)
    return P.run(list(gsz), pc, COEF, prec, state, itr_max, b, p, eps=eps)


# ---- scaling
SCALE_BOX = (33, 47, 61)
SCALE_K = 5
EPS_BELOW_REACH = 1e-300  # no residual of K iterations gets here: exactly K iterations run
# (precision, preconditioner): the shifts s at which K iterations must scale bit for bit (the issue's, and mg / mgrb checked the same way on
# the restatement), and the first s at which the restatement stops at iteration 1 (itr = 0, field untouched)
SCALED = {("f32", "jacobi"): (20, 40), ("f32", "none"): (30,), ("f64", "jacobi"): (40,), ("f64", "none"): (60,),
          ("f32", "mg"): (20, 40), ("f32", "mgrb"): (20, 40), ("f64", "mg"): (40,), ("f64", "mgrb"): (40,)}
STOPS = {("f32", "jacobi"): 70, ("f64", "none"): 70}  # beyond the threshold (stated with the cases above)
FIRST_STOP = {("f32", "none"): 68, ("f32", "jacobi"): 68, ("f32", "mg"): 69, ("f32", "mgrb"): 69,
              ("f64", "none"): 68, ("f64", "jacobi"): 68, ("f64", "mg"): 69, ("f64", "mgrb"): 69}  # the same in both: the threshold is absolute


def builtin_problem(prec):
    """(b, p) [i, j, k] of the test case cz_setup builds at SCALE_BOX (the oracle's set-up: the bytes the GPU driver's set-up leaves)"""
    k = PP.Kernels("oracle", prec)
    cz = PP.RB.CZ(k, wide=False, dots="exact")
    cz.setup(SCALE_BOX, COEF)
    return PP.unpad(cz.RHS), PP.unpad(cz.P)


def scaled_problem(prec, s, base=None):
    """the built-in problem (or `base`) times 2^-s, exactly: no datum underflows"""
    b, p = base if base is not None else builtin_problem(prec)
    f = real(prec)(2.0) ** real(prec)(-s)
    bs, ps = b * f, p * f
    assert bs.dtype == b.dtype and np.array_equal(bs / f, b) and np.array_equal(ps / f, p)
    return bs, ps
