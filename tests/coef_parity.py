"""Face coefficients for pcg, restated in numpy on the oracle (importable without a GPU): what tests/test_coef_oracle.py
checks on the CPU and tests/test_gpu_coef.py compares the GPU driver with.

The coefficients are three bricks [i, j, k] laid out as the velocity of project_parity: bx[i, j, k] lives on the face between cells i and
i + 1, faces 0 .. n0 - 2 (0-based here); entry n0 - 1 is never read; in a periodic direction face 0 is ignored and face n - 2 read in its
place (`imported` writes that alias into the padded copy, as the handle does); only faces at inner tangential indices are read.

The operator, each operation rounded once in the precision of the arrays, p's face layers filled by the state (periodic_parity.fill):
    per direction d   t_d = beta_d(c) (p(c + e_d) - p(c)) - beta_d(c - e_d) (p(c) - p(c - e_d))
    A p = (t_x + t_y) + t_z,     r = b - A p
    sub_grad          u(i, j, k) = u(i, j, k) - (bx(i, j, k) (p(i+1) - p(i))) scale,   v and w likewise
The identity (exact in small integers): div(u - beta grad p) == div u - A p.

The preconditioner is the constant-coefficient one of periodic_parity under the state, inside a diagonal scaling: z = s M^-1 (s r),
s = sqrt(6 / D), D = ((bx+ + bx-) + (by+ + by-)) + (bz+ + bz-) over the six faces of a cell -- the diagonal of the variable operator against
the 6 of the constant one.  `none` stays z = r.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_parity as M  # noqa: E402
import neumann_parity as N  # noqa: E402
import periodic_parity as P  # noqa: E402
import problem_parity as PP  # noqa: E402
import project_parity as J  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

STATES = J.STATES
PCG_STATES = {k: STATES[k] for k in ("dirichlet", "inflow", "closed", "channel")}


def _real(prec):
    return np.float32 if prec == "f32" else np.float64


def box(gsz):
    idx, _ = O.range_inner_index(list(gsz), [-1] * 6)
    return list(gsz), idx


# ---- seeded coefficient fields: three C-order bricks [i, j, k] of the precision
def _face_points(gsz, ax):
    """the coordinates in [0, 1] of the faces of direction ax (between cell c and c + 1 along ax), three arrays that broadcast"""
    pts = []
    for d in range(3):
        c = (np.arange(gsz[d]) + (0.5 if d == ax else 0.0)) / (gsz[d] - 1.0)
        pts.append(c.reshape([-1 if q == d else 1 for q in range(3)]))
    return pts


def random(gsz, prec, seed=0):
    """uniform in [0.5, 2]"""
    rng = np.random.default_rng(3000 + seed)
    return [(0.5 + 1.5 * rng.random(tuple(gsz))).astype(_real(prec)) for _ in range(3)]


def ints(gsz, prec, seed=0):
    """integers 1 .. 4"""
    rng = np.random.default_rng(3100 + seed)
    return [rng.integers(1, 5, size=tuple(gsz)).astype(_real(prec)) for _ in range(3)]


def smooth(gsz, prec, ratio):
    """ratio ** (a product of three sines, scaled to [0, 1]): between 1 and ratio, one period per direction"""
    out = []
    for ax in range(3):
        x, y, z = _face_points(gsz, ax)
        f = 0.5 * (1.0 + np.sin(2.0 * np.pi * x) * np.sin(2.0 * np.pi * y) * np.sin(2.0 * np.pi * z))
        out.append(np.ascontiguousarray(np.broadcast_to(float(ratio) ** f, tuple(gsz))).astype(_real(prec)))
    return out


def bubble(gsz, prec, ratio):
    """`ratio` on the faces whose centre lies in a ball of radius 0.25 about the middle of the box, 1 elsewhere: a sharp jump"""
    out = []
    for ax in range(3):
        x, y, z = _face_points(gsz, ax)
        inside = (x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2 < 0.25 ** 2
        out.append(np.ascontiguousarray(np.broadcast_to(np.where(inside, float(ratio), 1.0), tuple(gsz))).astype(_real(prec)))
    return out


def aniso(gsz, prec, ratio):
    """constant by direction: bx = bz = 1, by = 1 / ratio (a grid whose Y spacing is sqrt(ratio) times the others')"""
    R = _real(prec)
    return [np.full(tuple(gsz), v, dtype=R) for v in (1.0, 1.0 / float(ratio), 1.0)]


def ones(gsz, prec):
    return [np.ones(tuple(gsz), dtype=_real(prec)) for _ in range(3)]


FIELDS = {"random": lambda g, q: random(g, q), "smooth4": lambda g, q: smooth(g, q, 4), "smooth10": lambda g, q: smooth(g, q, 10),
          "bubble10": lambda g, q: bubble(g, q, 10), "bubble100": lambda g, q: bubble(g, q, 100), "bubble1000": lambda g, q: bubble(g, q, 1000),
          "aniso4": lambda g, q: aniso(g, q, 4), "ones": ones}


# ---- the operator
_AX = (1, 0, 2)  # the padded array's axis [j, i, k] of direction X, Y, Z


def imported(beta, per):
    """the handle's padded copies [j + 2, i + 2, k + 2] of bx, by, bz with face 0 of a periodic direction holding face n - 2"""
    out = []
    for d, b in enumerate(beta):
        B = PP.pad(np.ascontiguousarray(b))
        if per[d]:
            q = np.moveaxis(B, _AX[d], 0)
            q[O.GUIDE] = q[O.GUIDE + b.shape[d] - 2]
        out.append(B)
    return out


def _shift(a, ins, d, s):
    sl = list(ins)
    ax = _AX[d]
    sl[ax] = slice(ins[ax].start + s, ins[ax].stop + s)
    return a[tuple(sl)]


def apply(p, B, sz, idx):
    """A p at the cells of idx of the padded p (face layers filled) with the imported coefficients B"""
    R = p.dtype.type
    ins = M.inner(sz, idx)
    c = p[ins]
    t = []
    for d in range(3):
        up = np.multiply(B[d][ins], np.subtract(_shift(p, ins, d, 1), c, dtype=R), dtype=R)
        dn = np.multiply(_shift(B[d], ins, d, -1), np.subtract(c, _shift(p, ins, d, -1), dtype=R), dtype=R)
        t.append(np.subtract(up, dn, dtype=R))
    return np.add(np.add(t[0], t[1], dtype=R), t[2], dtype=R)


def scaling(B, sz, idx):
    """the padded array s: sqrt(6 / D) at the cells of idx, 0 elsewhere"""
    R = B[0].dtype.type
    ins = M.inner(sz, idx)
    pair = [np.add(B[d][ins], _shift(B[d], ins, d, -1), dtype=R) for d in range(3)]
    D = np.add(np.add(pair[0], pair[1], dtype=R), pair[2], dtype=R)
    s = np.zeros_like(B[0])
    s[ins] = np.sqrt(np.divide(R(6), D, dtype=R), dtype=R)
    return s


class Kernels(P.Kernels):
    """periodic_parity.Kernels whose blas_calc_ax / blas_calc_rk apply the variable operator after the fill (B: `imported`; None: the parent's)"""
    B = None

    def blas_calc_ax(self, ap, p, sz, idx, cf):
        if self.B is None:
            return super().blas_calc_ax(ap, p, sz, idx, cf)
        self.mirror(p, sz, idx)
        ap[M.inner(sz, idx)] = apply(p, self.B, sz, idx)

    def blas_calc_rk(self, r, p, b, sz, idx, cf):
        if self.B is None:
            return super().blas_calc_rk(r, p, b, sz, idx, cf)
        self.mirror(p, sz, idx)
        ins = M.inner(sz, idx)
        r[ins] = np.subtract(b[ins], apply(p, self.B, sz, idx), dtype=p.dtype.type)


class CZ(P.CZ):
    """periodic_parity.CZ whose preconditioner is s M^-1 (s .) while the kernels hold coefficients (scaled=False: M^-1 alone, the `plain`
    column of DESIGN.md §5.19)"""
    scaled = True

    def Preconditioner(self, xx, bb, pc):
        if self.k.B is None or not self.scaled:
            return super().Preconditioner(xx, bb, pc)
        ins = M.inner(self.size, self.idx)
        R = bb.dtype.type
        t = np.zeros_like(bb)
        t[ins] = np.multiply(self.s[ins], bb[ins], dtype=R)
        super().Preconditioner(xx, t, pc)
        z = np.multiply(self.s[ins], xx[ins], dtype=R)
        xx[...] = 0
        xx[ins] = z


def solver(gsz, coef, prec, state, beta, perturb=0, scaled=True):
    faces, per, closed = state
    assert P.solvable(faces, per, closed)
    k = Kernels("oracle", prec)
    k.faces, k.per = tuple(faces), tuple(per)
    cz = CZ(k, wide=False, dots="exact", perturb=perturb)
    cz.closed = bool(closed)
    cz.scaled = scaled
    cz.setup(list(gsz), coef)
    k.user = True
    if beta is not None:
        k.B = imported(beta, per)
        cz.s = scaling(k.B, cz.size, cz.idx)
    return cz, k


def run(gsz, pc, coef, prec, state, itr_max, b, p, beta, eps=None, perturb=0, scaled=True):
    """periodic_parity.run with the coefficients beta = (bx, by, bz) (None: that run itself)"""
    import closed_parity as C
    cz, k = solver(gsz, coef, prec, state, beta, perturb, scaled)
    cz.P, cz.RHS = PP.pad(p), PP.pad(b)
    closed = state[2]
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


def envelope_f64(gsz, pc, coef, state, itr_max, b, p, beta, eps=None):
    """FP64: the unperturbed run and the envelope of the runs with every dot (and sum) at either edge of its summation bound"""
    r = {q: run(gsz, pc, coef, "f64", state, itr_max, b, p, beta, eps=eps, perturb=q) for q in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr, [r[q].itr for q in (-1, 0, 1)]
    P0, h0 = r[0].P, np.array([v for _, v in r[0].history])
    E = np.maximum(np.abs(r[1].P - P0), np.abs(r[-1].P - P0))
    Eh = np.maximum(np.abs(np.array([v for _, v in r[1].history]) - h0), np.abs(np.array([v for _, v in r[-1].history]) - h0))
    return r[0], E, Eh


def premise_f32(gsz, pc, coef, state, itr_max, b, p, beta, eps=None):
    """the unperturbed FP32 run, after asserting that no dot lies within its summation bound of a rounding boundary and, in the closed mode,
    that the runs with every sum at either edge give its bits (periodic_parity.premise_f32)"""
    import cg_parity as CP
    r0 = run(gsz, pc, coef, "f32", state, itr_max, b, p, beta, eps=eps)
    f = CP.flips(r0, "f32")
    assert not f, f"dots within their summation bound of a float boundary {f[:4]}"
    if state[2]:
        for q in (-1, 1):
            rq = run(gsz, pc, coef, "f32", state, itr_max, b, p, beta, eps=eps, perturb=q)
            assert rq.itr == r0.itr and rq.history == r0.history, q
            assert rq.P.tobytes() == r0.P.tobytes() and rq.B.tobytes() == r0.B.tobytes(), q
    return r0


def residual(p, b, beta, state):
    """(r [i, j, k], sum r^2): r = b - A p at the inner cells and 0 elsewhere, of bricks p, b under the state"""
    sz, idx = box(p.shape)
    k = Kernels("oracle", "f32" if p.dtype == np.float32 else "f64")
    k.faces, k.per = tuple(state[0]), tuple(state[1])
    k.B = imported(beta, state[1])
    r = k.alloc(sz)
    k.blas_calc_rk(r, PP.pad(p), PP.pad(b), sz, idx, None)
    r = PP.unpad(r)
    return r, J.sumsq(r)


def sub_grad(vel, p, beta, per, scale, dtype):
    """project_parity.sub_grad with the coefficient: vel - (beta (p(+1) - p)) scale on the faces 0 .. n - 2 at inner tangential cells, face 0
    = face n - 2 in a periodic direction.  p [i, j, k] with its face layers filled (project_parity.fill_field)"""
    R = np.dtype(dtype).type
    p = np.asarray(p, dtype=R)
    out = []
    for ax, a in enumerate(vel):
        a = np.array(a, dtype=R)
        n = a.shape[ax]
        pi = J._inner(p, skip=ax)
        sl = tuple(slice(0, n - 1) if d == ax else slice(1, -1) for d in range(3))
        g = np.subtract(np.take(pi, np.arange(1, n), ax), np.take(pi, np.arange(0, n - 1), ax), dtype=R)
        g = np.multiply(np.asarray(beta[ax], dtype=R)[sl], g, dtype=R)
        g = np.multiply(g, R(scale), dtype=R)
        a[sl] = np.subtract(a[sl], g, dtype=R)
        if per[ax]:
            face = lambda f: tuple(f if d == ax else slice(1, -1) for d in range(3))  # noqa: E731
            a[face(0)] = a[face(n - 2)]
        out.append(a)
    return tuple(out)


def unread(gsz, per):
    """boolean masks [i, j, k] of the entries of bx, by, bz that the contract says are never read: entry n - 1, face 0 of a periodic
    direction, faces at boundary tangential indices"""
    out = []
    for ax in range(3):
        m = np.ones(tuple(gsz), dtype=bool)
        m[tuple(slice(1 if per[ax] else 0, gsz[ax] - 1) if d == ax else slice(1, -1) for d in range(3))] = False
        out.append(m)
    return out


def assembled(gsz, beta, state):
    """the operator as a dense matrix on the inner cells of a small box, C order [i, j, k], in double: column q = A e_q by `apply` with zero
    Dirichlet values"""
    sz, idx = box(gsz)
    n = [v - 2 for v in gsz]
    k = Kernels("oracle", "f64")
    k.faces, k.per = tuple(state[0]), tuple(state[1])
    k.B = imported([np.asarray(b, dtype=np.float64) for b in beta], state[1])
    A = np.zeros((n[0] * n[1] * n[2],) * 2)
    for q in range(A.shape[0]):
        e = np.zeros(tuple(gsz))
        e[1 + q // (n[1] * n[2]), 1 + (q // n[2]) % n[1], 1 + q % n[2]] = 1.0
        ap = k.alloc(sz)
        k.blas_calc_ax(ap, PP.pad(e), sz, idx, None)
        A[:, q] = PP.unpad(ap)[1:-1, 1:-1, 1:-1].ravel()
    return A


# ---- the projection end to end (tests/test_gpu_coef.py::test_project_end_to_end)
def project(gsz, pc, coef, prec, name, field, eps=None, itr_max=300):
    """project_parity.solve under coefficients: b = div vel, the solve, vel - beta grad p; dict(itr, ss0, ss1, ratio)"""
    state = STATES[name]
    R = _real(prec)
    vel = J.velocity(gsz, prec, 0, state)
    _, p0 = PP.problem(gsz, prec, 0)
    beta = FIELDS[field](gsz, prec)
    b, ss0 = J.div(vel, state[1], 1.0, R)
    o = run(list(gsz), pc, coef, prec, state, itr_max, b, p0, beta, eps=J.E2E_EPS[prec] if eps is None else eps)
    new = sub_grad(vel, PP.unpad(o.P), beta, state[1], 1.0, R)
    _, ss1 = J.div(new, state[1], 1.0, R)
    return dict(itr=o.itr, ss0=ss0, ss1=ss1, ratio=math.sqrt(ss1 / ss0), vel=new)


E2E_BOXES = J.E2E_BOXES
E2E_RUNS = J.E2E_RUNS
E2E_FIELDS = ("smooth4", "bubble10")

# ---- iterations to eps 1e-8 on the seeded problem at 33 x 47 x 61, FP64, Dirichlet faces, ItrMax 300: (field, run): (plain, scaled) -- plain
# is M^-1 alone, scaled s M^-1 s (tests/test_coef_oracle.py re-measures the scaled column and the constant operator)
COUNT_BOX = (33, 47, 61)
COUNT_EPS = 1e-8
COUNT_RUNS = [("mgrb", 1.2), ("mg", 0.8)]
from coef_measured import COUNTS, MEASURED  # noqa: E402  (recorded results: tests/coef_measured.py)

# the bar of tests/test_gpu_coef.py per (state, precision): 8 x the largest measured ratio of the state (the factor and the reason of
# project_parity.BARS)
BARS = {(s, q): 8.0 * max(v[0] for k, v in MEASURED.items() if k[3] == s and k[4] == q) for s in STATES for q in ("f64", "f32")}


# ---- the GPU PCG cases (tests/test_gpu_coef.py), chosen on the CPU (tests/test_coef_oracle.py: the FP32 premise, the FP64 envelope)
def case(gsz, pc, coef, prec, K, state, field, seed=0):
    return dict(gsz=tuple(gsz), pc=pc, coef=coef, prec=prec, K=K, state=state, field=field, seed=seed,
                id=f"pcg_{pc}_{'x'.join(map(str, gsz))}_{prec}_{state}_{field}_K{K}")


PCG_CASES = [
    case((9, 7, 12), "none", 0.8, "f32", 4, "dirichlet", "random"),
    case((9, 7, 12), "jacobi", 0.8, "f64", 4, "inflow", "smooth4"),
    case((9, 7, 12), "mg", 0.8, "f32", 3, "channel", "random"),
    case((9, 7, 12), "mgrb", 1.2, "f64", 3, "closed", "smooth4"),
    case((33, 47, 61), "none", 0.8, "f64", 5, "channel", "random"),
    case((33, 47, 61), "jacobi", 0.8, "f32", 4, "closed", "smooth4"),
    case((33, 47, 61), "mg", 0.8, "f64", 4, "inflow", "random"),
    case((33, 47, 61), "mgrb", 1.2, "f32", 4, "dirichlet", "smooth4"),
    case((40, 40, 1100), "jacobi", 0.8, "f32", 2, "dirichlet", "random"),
    case((40, 40, 1100), "mgrb", 1.2, "f64", 2, "inflow", "smooth4"),
]


def case_problem(c):
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    return b, p, FIELDS[c["field"]](c["gsz"], c["prec"])


def case_run(c, perturb=0):
    b, p, beta = case_problem(c)
    return run(c["gsz"], c["pc"], c["coef"], c["prec"], STATES[c["state"]], c["K"], b, p, beta, eps=1e-30, perturb=perturb)
