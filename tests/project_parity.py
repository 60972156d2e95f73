"""The projection step on a staggered velocity, restated in numpy (importable without a GPU): what
tests/test_project_oracle.py checks on the CPU and tests/test_gpu_project.py compares the GPU driver with.

The grid.  Arrays are bricks [i, j, k] (0-based here; the documents count from 1).  The cells are 0 .. n - 1, the inner cells 1 .. n - 2.
u[i, j, k] is the normal velocity on the face between cells i and i + 1, faces 0 .. n0 - 2; entry n0 - 1 is never read or written; v and w
are the same along j and k.  In a periodic direction cell 0 is cell n - 2 and cell n - 1 is cell 1, so face 0 is an alias of face n - 2:
`div` ignores face 0 and reads face n - 2 in its place, `sub_grad` writes face 0 with the value of face n - 2.  Nothing else depends on the
boundary state: a wall-normal velocity on a zero-flux face is the caller's datum and enters the divergence like any face; the gradient
leaves it alone because the mirror makes p(1) - p(0) = 0.

The operation order (each operation rounded once in `dtype`):
    div       dx = u(i) - u(i-1), dy = v(j) - v(j-1), dz = w(k) - w(k-1), d = (dx + dy) + dz, b = d * scale at the inner cells, 0 elsewhere
    sub_grad  u(i, j, k) = u(i, j, k) - (p(i+1, j, k) - p(i, j, k)) * scale  for faces 0 .. n0 - 2 at inner j, k; v, w likewise
The identity (exact in small integers, tests/test_project_oracle.py): with p's face layers filled by the state (periodic_parity.fill),
    div(u - grad p) == div u - (sum of the six neighbours - 6 p).
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_parity as C  # noqa: E402
import neumann_parity as N  # noqa: E402
import periodic_parity as P  # noqa: E402
import problem_parity as PP  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

INFLOW = (1, 0, 0, 0, 1, 1)  # inflow plane at X-, zero-flux Z-, Z+; Dirichlet X+, Y-, Y+
# the six states of the tests: (Neumann faces, periodic directions, closed)
STATES = {"dirichlet": (N.NONE, P.NOPER, False), "inflow": (INFLOW, P.NOPER, False), "closed": (C.SIX, P.NOPER, True),
          "px": P.STATES["px"], "channel": P.STATES["channel"], "triple": P.STATES["triple"]}
SMALL = [(9, 7, 12), (4, 5, 3), (3, 6, 4)]  # a direction of 3 cells: one inner cell, two faces; a periodic direction needs n >= 4


def fits(gsz, state):
    return all(not state[1][d] or gsz[d] >= 4 for d in range(3))


def _behind(a, axis, per):
    """a at face c - 1 for the inner cells c = 1 .. n - 2 of `axis` (face n - 2 in place of face 0 in a periodic direction)"""
    n = a.shape[axis]
    at = np.arange(0, n - 2)
    if per and n > 2:
        at[0] = n - 2
    return np.take(a, at, axis)


def _inner(a, skip=None):
    return a[tuple(slice(None) if d == skip else slice(1, -1) for d in range(3))]


def div_raw(vel, per, dtype):
    """the unscaled divergence at the inner cells, [n0 - 2, n1 - 2, n2 - 2]"""
    R = np.dtype(dtype).type
    d = []
    for ax, a in enumerate(vel):
        a = _inner(np.asarray(a, dtype=R), skip=ax)
        here = np.take(a, np.arange(1, a.shape[ax] - 1), ax)
        d.append(np.subtract(here, _behind(a, ax, per[ax]), dtype=R))
    return np.add(np.add(d[0], d[1], dtype=R), d[2], dtype=R)


def div(vel, per, scale, dtype):
    """(b, sumsq): b [i, j, k] = div * scale at the inner cells and 0 at the brick's other cells; sumsq = sum div^2 (unscaled), exact double
    squares, correctly rounded sum"""
    R = np.dtype(dtype).type
    d = div_raw(vel, per, dtype)
    b = np.zeros(np.asarray(vel[0]).shape, dtype=R)
    b[1:-1, 1:-1, 1:-1] = np.multiply(d, R(scale), dtype=R)
    return b, sumsq(d)


def sumsq(d):
    d = np.asarray(d, dtype=np.float64).ravel()
    return math.fsum(d * d)


def fill_field(p, state):
    """p [i, j, k] with the face layers the handle keeps under the state: the wrap, the mirror, or the values as given (Dirichlet)"""
    gsz = list(p.shape)
    idx, _ = O.range_inner_index(gsz, [-1] * 6)
    return PP.unpad(P.fill(PP.pad(p), gsz, idx, state[0], state[1]))


def sub_grad(vel, p, per, scale, dtype):
    """(u, v, w) new arrays: vel - grad p * scale on the faces 0 .. n - 2 at inner tangential cells, face 0 = face n - 2 in a periodic
    direction; every other element as given.  p [i, j, k] with its face layers filled (fill_field)"""
    R = np.dtype(dtype).type
    p = np.asarray(p, dtype=R)
    out = []
    for ax, a in enumerate(vel):
        a = np.array(a, dtype=R)  # (a copy)
        n = a.shape[ax]
        pi = _inner(p, skip=ax)
        g = np.subtract(np.take(pi, np.arange(1, n), ax), np.take(pi, np.arange(0, n - 1), ax), dtype=R)
        g = np.multiply(g, R(scale), dtype=R)
        sl = tuple(slice(0, n - 1) if d == ax else slice(1, -1) for d in range(3))
        a[sl] = np.subtract(a[sl], g, dtype=R)
        if per[ax]:
            face = lambda f: tuple(f if d == ax else slice(1, -1) for d in range(3))  # noqa: E731
            a[face(0)] = a[face(n - 2)]
        out.append(a)
    return tuple(out)


def face_fill(vel, per):
    """the alias written out: face 0 of a periodic direction = face n - 2 at inner tangential cells (what sub_grad leaves; div never reads it)"""
    out = []
    for ax, a in enumerate(vel):
        a = np.array(a)
        if per[ax]:
            face = lambda f: tuple(f if d == ax else slice(1, -1) for d in range(3))  # noqa: E731
            a[face(0)] = a[face(a.shape[ax] - 2)]
        out.append(a)
    return tuple(out)


def written(gsz, per):
    """boolean masks [i, j, k] of the elements of u, v, w that sub_grad writes"""
    out = []
    for ax in range(3):
        m = np.zeros(gsz, dtype=bool)
        lo = 1 if per[ax] else 0
        m[tuple(slice(lo, gsz[ax] - 1) if d == ax else slice(1, -1) for d in range(3))] = True
        if per[ax]:
            m[tuple(0 if d == ax else slice(1, -1) for d in range(3))] = True
        out.append(m)
    return out


def laplace(p):
    """sum of the six neighbours - 6 p at the inner cells of a filled p [i, j, k] (exact in small integers)"""
    c = p[1:-1, 1:-1, 1:-1]
    return (p[2:, 1:-1, 1:-1] + p[:-2, 1:-1, 1:-1] + p[1:-1, 2:, 1:-1] + p[1:-1, :-2, 1:-1] + p[1:-1, 1:-1, 2:] + p[1:-1, 1:-1, :-2]) - 6 * c


def boundary_flux(vel):
    """the net flux out of the inner box through its six faces (non-periodic box): sum over the faces n - 2 minus sum over the faces 0"""
    tot = 0.0
    for ax, a in enumerate(vel):
        a = _inner(np.asarray(a, dtype=np.float64), skip=ax)
        tot += math.fsum(np.take(a, a.shape[ax] - 2, ax).ravel()) - math.fsum(np.take(a, 0, ax).ravel())
    return tot


def velocity(gsz, prec, seed=0, state=None, integers=False, inflow=None):
    """a seeded staggered velocity [u, v, w], C order, in [-1, 1] (integers: in -4 .. 4).  With a closed state the wall-normal velocity on
    the faces of the directions that are not periodic is 0 (a compatible problem), or `inflow` on the X- face (a net flux)"""
    R = np.float32 if prec == "f32" else np.float64
    rng = np.random.default_rng(2000 + seed)
    vel = [(rng.integers(-4, 5, size=tuple(gsz)).astype(R) if integers else (rng.random(tuple(gsz)) * 2.0 - 1.0).astype(R)) for _ in range(3)]
    if state is not None and state[2]:
        for ax in range(3):
            if not state[1][ax]:
                for f in (0, gsz[ax] - 2):
                    vel[ax][tuple(f if d == ax else slice(None) for d in range(3))] = 0
    if inflow is not None:
        vel[0][0] = R(inflow)
    return vel


def solve(gsz, pc, coef, prec, state, vel, p0, eps, itr_max=300):
    """the projection on the restatement: b = div vel (scale 1), periodic_parity.run under the state (the closed mode projects b), then
    sub_grad.  Returns dict(itr, vel, p, b, ss0, ss1, rr): ss0 / ss1 = sum div^2 before / after, rr = sum (b - A p)^2 of the returned iterate
    against the unprojected b, by the oracle's blas_calc_rk"""
    b, ss0 = div(vel, state[1], 1.0, p0.dtype)
    o = P.run(list(gsz), pc, coef, prec, state, itr_max, b, p0, eps=eps)
    p = PP.unpad(o.P)
    new = sub_grad(vel, p, state[1], 1.0, p0.dtype)
    _, ss1 = div(new, state[1], 1.0, p0.dtype)
    k = P.kernels(prec, state[0], state[1])
    sz = list(gsz)
    idx, _ = O.range_inner_index(sz, [-1] * 6)
    r = k.alloc(sz)
    k.blas_calc_rk(r, o.P, PP.pad(b), sz, idx, np.array([1, 1, 1, 1, 1, 1, 6], dtype=k.real))
    return dict(itr=o.itr, vel=new, p=p, b=b, ss0=ss0, ss1=ss1, rr=sumsq(PP.unpad(r)[1:-1, 1:-1, 1:-1]), res=o.res)


# ---- the end-to-end cases: `pcg mgrb 1.2` and `pcg mg 0.8`, eps 1e-10 (FP32: 1e-5), the seeded velocity (compatible in the singular states)
# and problem_parity.problem's field (its outer layers are the Dirichlet values)
E2E_BOXES = [(33, 47, 61), (34, 34, 34)]
E2E_RUNS = [("mgrb", 1.2), ("mg", 0.8)]
E2E_EPS = {"f64": 1e-10, "f32": 1e-5}


def e2e(gsz, pc, coef, prec, name):
    state = STATES[name]
    vel = velocity(gsz, prec, 0, state)
    _, p0 = PP.problem(gsz, prec, 0)
    return solve(gsz, pc, coef, prec, state, vel, p0, E2E_EPS[prec])


# ||div after||_2 / ||div before||_2 of the restatement and its iteration count, per (box, run, state, precision), as `e2e` gives them
# (tests/test_project_oracle.py re-measures the (33, 47, 61) rows).  The solve stops at an RMS residual below eps and the seeded divergence has
# an RMS of about 1.41, so a converged solve gives at most eps / 1.41 = 7.1e-11 (FP32: 7.1e-6); a lost or misplaced face gives a ratio of
# order 1.
MEASURED = {  # (box, run, state, precision): (ratio, iterations)
    ((33, 47, 61), 'mgrb', 'dirichlet', 'f64'): (1.693e-11, 12),
    ((33, 47, 61), 'mgrb', 'inflow', 'f64'): (1.017e-11, 13),
    ((33, 47, 61), 'mgrb', 'closed', 'f64'): (2.632e-11, 10),
    ((33, 47, 61), 'mgrb', 'px', 'f64'): (4.883e-11, 12),
    ((33, 47, 61), 'mgrb', 'channel', 'f64'): (4.425e-11, 10),
    ((33, 47, 61), 'mgrb', 'triple', 'f64'): (2.608e-11, 10),
    ((33, 47, 61), 'mg', 'dirichlet', 'f64'): (6.614e-11, 19),
    ((33, 47, 61), 'mg', 'inflow', 'f64'): (3.267e-11, 20),
    ((33, 47, 61), 'mg', 'closed', 'f64'): (3.061e-11, 16),
    ((33, 47, 61), 'mg', 'px', 'f64'): (3.069e-11, 20),
    ((33, 47, 61), 'mg', 'channel', 'f64'): (6.476e-11, 16),
    ((33, 47, 61), 'mg', 'triple', 'f64'): (3.586e-11, 17),
    ((34, 34, 34), 'mgrb', 'dirichlet', 'f64'): (7.133e-12, 10),
    ((34, 34, 34), 'mgrb', 'inflow', 'f64'): (3.043e-11, 10),
    ((34, 34, 34), 'mgrb', 'closed', 'f64'): (4.937e-11, 9),
    ((34, 34, 34), 'mgrb', 'px', 'f64'): (1.612e-11, 10),
    ((34, 34, 34), 'mgrb', 'channel', 'f64'): (5.439e-11, 9),
    ((34, 34, 34), 'mgrb', 'triple', 'f64'): (1.780e-11, 9),
    ((34, 34, 34), 'mg', 'dirichlet', 'f64'): (3.929e-11, 17),
    ((34, 34, 34), 'mg', 'inflow', 'f64'): (6.609e-11, 18),
    ((34, 34, 34), 'mg', 'closed', 'f64'): (4.127e-11, 15),
    ((34, 34, 34), 'mg', 'px', 'f64'): (1.694e-11, 18),
    ((34, 34, 34), 'mg', 'channel', 'f64'): (5.032e-11, 15),
    ((34, 34, 34), 'mg', 'triple', 'f64'): (4.981e-11, 14),
    ((33, 47, 61), 'mgrb', 'dirichlet', 'f32'): (1.549e-06, 6),
    ((33, 47, 61), 'mgrb', 'inflow', 'f32'): (6.064e-06, 6),
    ((33, 47, 61), 'mgrb', 'closed', 'f32'): (1.699e-06, 5),
    ((33, 47, 61), 'mgrb', 'px', 'f32'): (3.113e-06, 6),
    ((33, 47, 61), 'mgrb', 'channel', 'f32'): (1.808e-06, 5),
    ((33, 47, 61), 'mgrb', 'triple', 'f32'): (1.383e-06, 5),
    ((33, 47, 61), 'mg', 'dirichlet', 'f32'): (5.608e-06, 9),
    ((33, 47, 61), 'mg', 'inflow', 'f32'): (2.873e-06, 10),
    ((33, 47, 61), 'mg', 'closed', 'f32'): (3.144e-06, 8),
    ((33, 47, 61), 'mg', 'px', 'f32'): (6.520e-06, 9),
    ((33, 47, 61), 'mg', 'channel', 'f32'): (2.474e-06, 8),
    ((33, 47, 61), 'mg', 'triple', 'f32'): (4.544e-06, 8),
    ((34, 34, 34), 'mgrb', 'dirichlet', 'f32'): (1.063e-06, 5),
    ((34, 34, 34), 'mgrb', 'inflow', 'f32'): (1.837e-06, 5),
    ((34, 34, 34), 'mgrb', 'closed', 'f32'): (9.236e-07, 5),
    ((34, 34, 34), 'mgrb', 'px', 'f32'): (1.286e-06, 5),
    ((34, 34, 34), 'mgrb', 'channel', 'f32'): (6.441e-07, 5),
    ((34, 34, 34), 'mgrb', 'triple', 'f32'): (6.353e-07, 5),
    ((34, 34, 34), 'mg', 'dirichlet', 'f32'): (4.558e-06, 8),
    ((34, 34, 34), 'mg', 'inflow', 'f32'): (5.248e-06, 9),
    ((34, 34, 34), 'mg', 'closed', 'f32'): (2.371e-06, 8),
    ((34, 34, 34), 'mg', 'px', 'f32'): (4.711e-06, 8),
    ((34, 34, 34), 'mg', 'channel', 'f32'): (2.818e-06, 8),
    ((34, 34, 34), 'mg', 'triple', 'f32'): (3.890e-06, 7),
}
# the bar of tests/test_gpu_project.py per (state, precision): 8 x the largest measured ratio of the state (8: the GPU's dots are double
# sums in another order, so its iterate differs from the restatement's at rounding level and the stopping residual with it)
BARS = {(s, q): 8.0 * max(v[0] for k, v in MEASURED.items() if k[2] == s and k[3] == q) for s in STATES for q in ("f64", "f32")}
