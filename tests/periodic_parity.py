"""Periodic directions for pcg, restated on the oracle (importable without a GPU): what tests/test_periodic_oracle.py checks
on the CPU and tests/test_gpu_periodic.py compares the GPU driver with.

The state is three flags (X, Y, Z) beside the six Neumann flags of neumann_parity and the closed mode of closed_parity.  The rules:

* level 0 keeps the unit-coefficient kernels and D = 6.  In a periodic direction the two face layers hold the wrap, p(1) = p(size-1) and
  p(size) = p(2) over the inner box, re-made before every kernel that reads the field's neighbours (`fill`: the wraps and, in the other
  directions, the mirrors of neumann_parity).  In a periodic direction the Neumann flags are ignored;
* levels >= 1: across the seam the Galerkin operator has the ordinary link Wx = Ey Ez between the last and the first point, carried by wrapping
  the level array's ghost layer before every kernel that reads the iterate's neighbours (`levels` exchanges mg_parity.pad for the wrapped
  one and mg_parity.weights for the per-level diagonal).  A level of ONE point in a periodic direction has no link there: both mask bits
  (c = 0) and a zero ghost layer.  D stays 2 (Wx + Wy + Wz) otherwise;
* red-black: mgrb_parity.sweep computes the relaxed update of every point from the array as it is before the colour sweep and keeps it at the
  points of the colour.  With the wrapped pad that IS the seam rule: on an even periodic extent the seam points have opposite colours, on an
  odd one they share a colour and read each other's value from before the sweep.

The solver class is closed_parity.CZ (neumann_parity's loop; with `closed` the three projections) with the V-cycles routed through `apply`.
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cg_parity as CP  # noqa: E402
import closed_parity as C  # noqa: E402
import mg_parity as M  # noqa: E402
import mgrb_parity as RB  # noqa: E402
import neumann_parity as N  # noqa: E402
import problem_parity as PP  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

NOPER = (0, 0, 0)
PX, PY, PZ, PXZ, PYZ, PXYZ = (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)
Y_MINUS = (0, 0, 1, 0, 0, 0)
# the states of the tests: (Neumann faces, periodic directions, closed)
STATES = {"px": (N.NONE, PX, False), "pxz_ym": (Y_MINUS, PXZ, False), "channel": (C.SIX, PXZ, True), "triple": (C.SIX, PXYZ, True)}
_AXIS = (1, 0, 2)  # the array axis [j, i, k] of direction X, Y, Z

_WRAP = [NOPER]  # the wrap flags of the level whose weights were asked for last (mg_parity.smooth / residual ask right before they pad)


def bits(per):
    return sum(1 << d for d in range(3) if per[d])


def effective(faces, per):
    """the Neumann flags that count: none in a periodic direction"""
    return tuple(0 if per[f >> 1] else (1 if faces[f] else 0) for f in range(6))


def solvable(faces, per, closed):
    """the setters' one rule: with the closed mode off, some face of a direction that is not periodic is a Dirichlet face"""
    return bool(closed) or any(not per[d] and not (faces[2 * d] and faces[2 * d + 1]) for d in range(3))


def fill(p, sz, idx, faces, per):
    """the face layers of the padded array p [j + 2, i + 2, k + 2], in place: the wrap in the periodic directions (both faces physical on the
    brick), the mirror on the Neumann faces of the others.  Every source is an inner layer, so the order does not matter"""
    js, is_, ks = M.inner(sz, idx)
    if per[0]:
        assert idx[0] == 2 and idx[1] == sz[0] - 1
        p[js, is_.start - 1, ks] = p[js, is_.stop - 1, ks]
        p[js, is_.stop, ks] = p[js, is_.start, ks]
    if per[1]:
        assert idx[2] == 2 and idx[3] == sz[1] - 1
        p[js.start - 1, is_, ks] = p[js.stop - 1, is_, ks]
        p[js.stop, is_, ks] = p[js.start, is_, ks]
    if per[2]:
        assert idx[4] == 2 and idx[5] == sz[2] - 1
        p[js, is_, ks.start - 1] = p[js, is_, ks.stop - 1]
        p[js, is_, ks.stop] = p[js, is_, ks.start]
    return N.mirror(p, sz, idx, effective(faces, per))


def kinds(faces, per):
    """czhip_fill_faces_async's argument for the state"""
    return [2 if per[f >> 1] else (1 if faces[f] else 0) for f in range(6)]


class Kernels(N.Kernels):
    """neumann_parity.Kernels whose neighbour-reading kernels fill (wrap and mirror) their input first"""
    per = NOPER

    def mirror(self, p, sz, idx):
        if any(self.per):
            fill(p, sz, idx, self.faces, self.per)
        else:
            super().mirror(p, sz, idx)


def level_state(n0, level, faces, per):
    """(the six mask bits of the level, its wrap flags): a periodic direction of two or more points wraps and has no mask bit, one of a
    single point takes both mask bits and does not wrap; the other directions keep their Neumann flags"""
    dims = M.level_dims(n0)[level]
    f, w = list(effective(faces, per)), [0, 0, 0]
    for d in range(3):
        if per[d]:
            if dims[d] >= 2:
                w[d] = 1
            else:
                f[2 * d] = f[2 * d + 1] = 1
    return tuple(f), tuple(w)


def wrapped_pad(a):
    """mg_parity.pad with the ghost layers of the flagged directions holding the wrap (edges and corners are not read)"""
    p = np.pad(a, 1)
    for d in range(3):
        if _WRAP[0][d]:
            ax = _AXIS[d]
            q = np.moveaxis(p, ax, 0)
            inner = (slice(1, -1), slice(1, -1))
            q[0][inner] = q[-2][inner]
            q[-1][inner] = q[1][inner]
    return p


@contextlib.contextmanager
def levels(faces, per):
    """inside: mg_parity's and mgrb_parity's coarse cycles take the per-level diagonal and the wrapped ghost layers"""
    keep = M.weights, M.pad

    def weights(n0, level, R):
        f, w = level_state(n0, level, faces, per)
        _WRAP[0] = w  # (level 0 too: the cycles never ask for it, `level_operator` does)
        return N.weights(n0, level, R, f)

    M.weights, M.pad = weights, wrapped_pad
    try:
        yield
    finally:
        M.weights, M.pad = keep
        _WRAP[0] = NOPER


def apply(kind, k, r, sz, idx, omg):
    """z = V_0(r) of `mg` | `mgrb` on full S3D arrays under the state of k (a `Kernels` of this file): neumann_parity.apply with the fill at
    level 0 and `levels` on the coarse ones"""
    R = k.real
    cf = np.array([1, 1, 1, 1, 1, 1, 6], dtype=R)
    n0 = M.n0_of(idx)
    ins = M.inner(sz, idx)
    z, wk2 = k.alloc(sz), k.alloc(sz)

    def pair(post):
        for _ in range(2):
            if kind == "mg":
                k.jacobi(z, sz, idx, cf, R(omg), r, wk2)
            else:
                RB.fine_iteration(k, z, r, sz, idx, omg, post)

    with levels(k.faces, k.per):
        if len(M.level_dims(n0)) == 1:
            for s in range(4):
                pair(s >= 2)
            return z
        pair(False)
        k.mirror(z, sz, idx)
        cycle = M.vcycle if kind == "mg" else RB.vcycle
        xc = cycle(N.restrict0(z, r, sz, idx), 1, n0, R(omg))
        z[ins] = M.prolong(z[ins], xc)
        pair(True)
    return z


class CZ(C.CZ):
    """closed_parity.CZ whose V-cycles are those of this file (k: a `Kernels` of this file)"""

    def Preconditioner(self, xx, bb, pc):
        if not (self._mg or self._mgrb):
            return super(N.CZ, self).Preconditioner(xx, bb, pc)  # jacobi: the 8 sweeps, each filling its input
        xx[...] = apply("mgrb" if self._mgrb else "mg", self.k, bb, self.size, self.idx, self.ac1)
        self.cycles += 1


def kernels(prec, faces, per):
    k = Kernels("oracle", prec)
    k.faces, k.per = tuple(faces), tuple(per)
    return k


def solver(gsz, coef, prec, faces, per, closed=False, perturb=0):
    assert solvable(faces, per, closed)
    k = kernels(prec, faces, per)
    cz = CZ(k, wide=False, dots="exact", perturb=perturb)
    cz.closed = bool(closed)
    cz.setup(list(gsz), coef)
    k.user = True
    return cz, k


def run(gsz, pc, coef, prec, state, itr_max, b, p, eps=None, perturb=0):
    """`pcg itr_max coef pc` on the problem (b, p) [i, j, k] under state = (faces, per, closed): O.Result, P with the fills in place (no flag:
    the bytes of neumann_parity.run / closed_parity.run)"""
    faces, per, closed = state
    cz, k = solver(gsz, coef, prec, faces, per, closed, perturb)
    cz.P, cz.RHS = PP.pad(p), PP.pad(b)
    mb, tol_b = C.project(cz.RHS, cz.size, cz.idx, perturb, tol=True) if closed else (None, None)
    k.mirror(cz.P, cz.size, cz.idx)
    if eps is not None:
        cz.eps = eps
    cz.cycles = 0
    itr, res = cz.PCG(cz.P, cz.RHS, itr_max, pc)
    k.mirror(cz.P, cz.size, cz.idx)
    out = O.Result(itr=itr, res=res, history=cz.history, P=cz.P, dot_log=cz.dot_log)
    out.cycles = cz.cycles
    if closed:
        out.means = [mb] + cz.means[1:]
        out.mean_tol = [tol_b, None, cz.tol_x]
        out.sum_log = cz.sum_log
        out.B = cz.RHS
    return out


def envelope_f64(gsz, pc, coef, state, itr_max, b, p, eps=None):
    """FP64: the unperturbed run and the envelope of the runs with every dot (and sum) at either edge of its summation bound"""
    r = {q: run(gsz, pc, coef, "f64", state, itr_max, b, p, eps=eps, perturb=q) for q in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr, [r[q].itr for q in (-1, 0, 1)]
    P0, h0 = r[0].P, np.array([v for _, v in r[0].history])
    E = np.maximum(np.abs(r[1].P - P0), np.abs(r[-1].P - P0))
    Eh = np.maximum(np.abs(np.array([v for _, v in r[1].history]) - h0), np.abs(np.array([v for _, v in r[-1].history]) - h0))
    return r[0], E, Eh


def premise_f32(gsz, pc, coef, state, itr_max, b, p, eps=None):
    """the unperturbed FP32 run, after asserting that no dot lies within its summation bound of a rounding boundary and, in the closed mode,
    that the runs with every sum at either edge give its bits (closed_parity.premise_f32)"""
    r0 = run(gsz, pc, coef, "f32", state, itr_max, b, p, eps=eps)
    f = CP.flips(r0, "f32")
    assert not f, f"dots within their summation bound of a float boundary {f[:4]}"
    if state[2]:
        for q in (-1, 1):
            rq = run(gsz, pc, coef, "f32", state, itr_max, b, p, eps=eps, perturb=q)
            assert rq.itr == r0.itr and rq.history == r0.history, q
            assert rq.P.tobytes() == r0.P.tobytes() and rq.B.tobytes() == r0.B.tobytes(), q
    return r0


def assembled(gsz, faces, per):
    """the operator as a dense matrix on the inner cells of a small box, C order [i, j, k]: neumann_parity.assembled with a link of 1 across
    the seam of a periodic direction (two inner points: both links reach the same neighbour, 2)"""
    n = [v - 2 for v in gsz]
    A = np.zeros((n[0] * n[1] * n[2],) * 2)
    at = lambda i, j, k: (i * n[1] + j) * n[2] + k  # noqa: E731
    f = effective(faces, per)
    for i in range(n[0]):
        for j in range(n[1]):
            for k in range(n[2]):
                q, c = at(i, j, k), (i, j, k)
                A[q, q] += -6.0
                for d in range(3):
                    for s in (-1, 1):
                        m = list(c)
                        m[d] += s
                        if 0 <= m[d] < n[d]:
                            A[q, at(*m)] += 1.0
                        elif per[d]:
                            m[d] %= n[d]
                            A[q, at(*m)] += 1.0
                        elif f[2 * d + (s > 0)]:
                            A[q, q] += 1.0
    return A


def prolongation(n0, level):
    """the aggregation P of level `level` as a dense 0 / 1 matrix, (level-0 points) x (level points), both in C order [i, j, k]"""
    dims = M.level_dims(n0)[level]
    Pm = np.zeros((n0[0] * n0[1] * n0[2], dims[0] * dims[1] * dims[2]))
    for i in range(n0[0]):
        for j in range(n0[1]):
            for k in range(n0[2]):
                I, J, K = i >> level, j >> level, k >> level
                Pm[(i * n0[1] + j) * n0[2] + k, (I * dims[1] + J) * dims[2] + K] = 1.0
    return Pm


def level_operator(n0, level, faces, per):
    """the level's operator as the rules of this file state it (the residual of the restated kernels, A x = -(residual of x with b = 0)), dense,
    C order [I, J, K]"""
    dims = M.level_dims(n0)[level]
    n = dims[0] * dims[1] * dims[2]
    A = np.zeros((n, n))
    with levels(faces, per):
        for q in range(n):
            e = np.zeros(n)
            e[q] = 1.0
            x = np.ascontiguousarray(e.reshape(dims).transpose(1, 0, 2))  # [j, i, k]
            r = M.residual(x, np.zeros_like(x), level, n0)
            A[:, q] = -np.ascontiguousarray(r.transpose(1, 0, 2)).ravel()
    return A


def manufactured(gsz, faces, per):
    """(u, b, p) in FP64: a smooth u on the inner cells that is periodic in the flagged directions (period = the inner extent), filled onto
    the periodic and Neumann faces and kept on the Dirichlet ones; b = A u by the oracle's blas_calc_ax on the filled field; p = u on the
    faces and zero inside"""
    k = kernels("f64", faces, per)
    ax = []
    for d in range(3):
        n = gsz[d] - 2
        t = (np.arange(gsz[d]) - 1.0) / n if per[d] else np.linspace(0.0, 1.0, gsz[d])
        ax.append(t)
    x, y, z = ax
    fx = np.sin(2.0 * np.pi * x) if per[0] else np.sin(2.0 * x)
    fy = np.cos(2.0 * np.pi * y) if per[1] else np.cos(1.5 * y)
    fz = np.sin(4.0 * np.pi * z) + 1.5 if per[2] else np.exp(0.5 * z)
    u = np.ascontiguousarray(fx[:, None, None] * fy[None, :, None] * fz[None, None, :] + fy[None, :, None] * fz[None, None, :])
    sz = list(gsz)
    idx, _ = O.range_inner_index(sz, [-1] * 6)
    U = PP.pad(u)
    fill(U, sz, idx, faces, per)
    AU = k.alloc(sz)
    k.blas_calc_ax(AU, U, sz, idx, np.array([1, 1, 1, 1, 1, 1, 6], dtype=np.float64))
    u = PP.unpad(U)
    p = u.copy()
    p[1:-1, 1:-1, 1:-1] = 0.0
    return u, PP.unpad(AU), p


def refine(b, p, state, tol=1e-10, max_outer=20, inner_eps=None, inner=("mgrb", 1.2)):
    """neumann_parity.refine under a state without the closed mode: (outer steps taken or 0, history, p, ratios)"""
    import refine_parity as RP
    faces, per, closed = state
    assert not closed
    inner_eps = RP.INNER_EPS if inner_eps is None else inner_eps
    gsz = list(p.shape)
    k = kernels("f64", faces, per)
    idx, _ = O.range_inner_index(gsz, [-1] * 6)
    cf = np.array([1, 1, 1, 1, 1, 1, 6], dtype=np.float64)
    B = PP.pad(b.astype(np.float64))

    def residual(q):
        Q, r = PP.pad(q), k.alloc(gsz)
        k.blas_calc_rk(r, Q, B, gsz, idx, cf)
        return PP.unpad(r), PP.unpad(Q)

    p = p.astype(np.float64).copy()
    npts = int(np.prod([n - 2 for n in gsz]))
    ss0 = RP.sumsq(residual(p)[0])
    ss, hist, ratios, its, step = ss0, [], [], 0, 0
    while True:
        scale = RP.scale_of(ss, npts)
        r, p = residual(p)
        ss = RP.sumsq(r)
        rel = float(np.sqrt(ss) / np.sqrt(ss0))
        ratios.append(rel)
        if step > 0:
            hist.append((step, rel, its))
        if np.sqrt(ss) <= tol * np.sqrt(ss0):
            return step, hist, p, ratios
        if step == max_outer:
            return 0, hist, p, ratios
        r32 = RP.scaled(r, scale, np.float32)
        o = run(gsz, inner[0], inner[1], "f32", state, 1000, r32, np.zeros(gsz, dtype=np.float32), eps=inner_eps)
        its = o.itr
        p = RP.add(p, PP.unpad(o.P), 1.0 / scale)
        step += 1


# ---- the GPU cases (tests/test_gpu_periodic.py), chosen on the CPU (tests/test_periodic_oracle.py: FP32 premise of bit equality, counts)
def case(gsz, pc, coef, prec, K, state, seed=0):
    return dict(gsz=tuple(gsz), pc=pc, coef=coef, prec=prec, K=K, state=state, seed=seed,
                id=f"pcg_{pc}_{'x'.join(map(str, gsz))}_{prec}_{state}_K{K}")


PCG_CASES = [
    case((9, 7, 12), "none", 0.8, "f32", 4, "px"),
    case((9, 7, 12), "jacobi", 0.8, "f64", 4, "pxz_ym"),
    case((9, 7, 12), "mg", 0.8, "f32", 3, "pxz_ym"),
    case((9, 7, 12), "mgrb", 1.2, "f64", 3, "px"),
    case((33, 47, 61), "none", 0.8, "f64", 5, "pxz_ym"),
    case((33, 47, 61), "jacobi", 0.8, "f32", 4, "px"),
    case((33, 47, 61), "mg", 0.8, "f64", 4, "px"),
    case((33, 47, 61), "mgrb", 1.0, "f32", 4, "pxz_ym"),
]


def case_run(c, itr_max=None, perturb=0):
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    return run(c["gsz"], c["pc"], c["coef"], c["prec"], STATES[c["state"]], itr_max or c["K"], b, p, eps=1e-30, perturb=perturb)


# iterations to eps 1e-5 on the seeded problem at 33 x 47 x 61, FP64 (tests/test_periodic_oracle.py::test_oracle_iteration_counts records them;
# the singular states on the seeded incompatible b, projected, ItrMax 300)
COUNT_BOX = (33, 47, 61)
COUNT_RUNS = [("none", 0.8), ("jacobi", 0.8), ("mg", 0.8), ("mgrb", 0.8), ("mgrb", 1.2)]
COUNT_STATES = {"px": (N.NONE, PX, False), "pxz": (N.NONE, PXZ, False), "channel": STATES["channel"], "triple": STATES["triple"]}
COUNTS = {("px", "none", 0.8): 104, ("px", "jacobi", 0.8): 28, ("px", "mg", 0.8): 9, ("px", "mgrb", 0.8): 7, ("px", "mgrb", 1.2): 6,
          ("pxz", "none", 0.8): 114, ("pxz", "jacobi", 0.8): 31, ("pxz", "mg", 0.8): 9, ("pxz", "mgrb", 0.8): 7, ("pxz", "mgrb", 1.2): 5,
          ("channel", "none", 0.8): 120, ("channel", "jacobi", 0.8): 32, ("channel", "mg", 0.8): 7, ("channel", "mgrb", 0.8): 6,
          ("channel", "mgrb", 1.2): 4,
          ("triple", "none", 0.8): 89, ("triple", "jacobi", 0.8): 23, ("triple", "mg", 0.8): 8, ("triple", "mgrb", 0.8): 6,
          ("triple", "mgrb", 1.2): 4}

# decomposed runs on the LOCAL transport (case, division, state): solved to eps 1e-5 within ItrMax 100
DECOMP = [(dict(gsz=(32, 36, 40), prec="f32", pc="jacobi", coef=0.8, id="jacobi_32x36x40_f32_2x2x1_pz"), (2, 2, 1), (N.NONE, PZ, False)),
          (dict(gsz=(32, 36, 40), prec="f64", pc="mg", coef=0.8, id="mg_32x36x40_f64_2x1x2_py"), (2, 1, 2), (N.NONE, PY, False))]
