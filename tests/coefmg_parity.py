"""Face coefficients inside the multigrid hierarchy (cz_set_coef_mg), restated in numpy on the oracle (importable without a GPU; DESIGN.md
§5.20): what tests/test_coefmg_oracle.py checks on the CPU and tests/test_gpu_coefmg.py compares the GPU driver with.

The levels, the walk, the restriction tree and the prolongation are those of mg_parity, the smoothers those of mg_parity (`mg`) and
mgrb_parity (`mgrb`), the fills those of periodic_parity.  Only the weights change.

* Level l has face-weight arrays X, Y, Z and a diagonal D.  Arrays here are [j, i, k] as in mg_parity; X has one more entry along i (index
  I + 1 holds the link between points I and I + 1, I = -1 .. n - 1: entries 0 and n are the box's two faces), Y along j, Z along k.
* Level 0's weights are the handle's imported coefficients as they are (coef_parity.imported: face 0 of a periodic direction holds face
  n - 2).  Its iterate is filled as the constant cycle's level 0: mirror on Neumann faces, wrap in periodic directions, zero on Dirichlet faces.
* Coarsening: X_{l+1}(I, J, K) = (X(f, 2J, 2K) + X(f, 2J, 2K+1)) + (X(f, 2J+1, 2K) + X(f, 2J+1, 2K+1)), f = -1 for I = -1, else
  min(2I + 1, n_l - 1); absent children drop out; Y and Z likewise, the faster-running tangential direction paired first (k before i before j).
  A box face that carries no link at the COARSE level is stored as 0: a Neumann face of a direction that is not periodic, and both faces of
  a periodic direction in which the coarse level has one point (the mask bits of periodic_parity.level_state).
* D = ((X(I) + X(I-1)) + (Y(J) + Y(J-1))) + (Z(K) + Z(K-1)) on the stored weights, at every level.
* ss = X(I) u(I+1) + X(I-1) u(I-1) + Y(J) u(J+1) + Y(J-1) u(J-1) + Z(K) u(K+1) + Z(K-1) u(K-1), left to right;
  sweep pn = pp + ((ss - bb) / D - pp) omg; residual b - (ss - D x); every operation rounded once in the precision of the arrays.
* Levels >= 1 wrap the iterate where the constant cycle does and need no mirror: the zeroed weights drop the link.
* Bad values: every weight and D of levels >= 1 that is not finite and positive is counted (a stored zero of a dropped link is not).
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cg_parity as CP  # noqa: E402
import coef_parity as K  # noqa: E402
import mg_parity as M  # noqa: E402
import mgrb_parity as RB  # noqa: E402
import periodic_parity as P  # noqa: E402
import problem_parity as PP  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

FIELDS = K.FIELDS
PCG_STATES = K.PCG_STATES
_NORMAL = (1, 0, 2)      # the array axis [j, i, k] of direction X, Y, Z
_TANGENT = ((2, 0), (2, 1), (1, 0))  # per direction: the tangential axes in pairing order (k before i before j)


class Level:
    """one level's weights: W[d] along its direction has n + 1 entries, D the diagonal, mirrors the six fill flags of level 0 (none on
    levels >= 1), wraps the three wrap flags"""

    def __init__(self, W, mirrors, wraps, cut=(0,) * 6):
        self.W, self.mirrors, self.wraps, self.cut = W, tuple(mirrors), tuple(wraps), tuple(cut)
        R = W[0].dtype.type
        pair = [np.add(_take(W[d], d, slice(1, None)), _take(W[d], d, slice(None, -1)), dtype=R) for d in range(3)]
        self.D = np.add(np.add(pair[0], pair[1], dtype=R), pair[2], dtype=R)

    @property
    def shape(self):
        return self.D.shape


def _take(a, d, sl):
    s = [slice(None)] * 3
    s[_NORMAL[d]] = sl
    return a[tuple(s)]


def level0(B, sz, idx, faces, per):
    """level 0 from the imported padded copies"""
    ins = M.inner(sz, idx)
    W = []
    for d in range(3):
        s = list(ins)
        ax = _NORMAL[d]
        s[ax] = slice(ins[ax].start - 1, ins[ax].stop)
        W.append(np.ascontiguousarray(B[d][tuple(s)]))
    return Level(W, P.effective(faces, per), per)


def coarsen(F, mask, wraps):
    """the next level's weights from level F's; mask: the six flags of the coarse level's faces that carry no link"""
    W = []
    for d in range(3):
        ax = _NORMAL[d]
        nf = F.shape[ax]
        nc = (nf + 1) // 2
        f = np.array([0] + [min(2 * I + 1, nf - 1) + 1 for I in range(nc)])
        a = np.take(F.W[d], f, axis=ax)
        for t in _TANGENT[d]:
            a = M._pair(a, t)
        a = np.ascontiguousarray(a)
        if mask[2 * d]:
            _take(a, d, 0)[...] = 0
        if mask[2 * d + 1]:
            _take(a, d, -1)[...] = 0
        W.append(a)
    return Level(W, (0,) * 6, wraps, mask)


def hierarchy(beta, gsz, state, prec=None):
    """every level of the box under the state (faces, per, closed), from the coefficient bricks beta [i, j, k]"""
    faces, per, _ = state
    sz, idx = K.box(gsz)
    if prec is not None:
        beta = [np.asarray(b, dtype=K._real(prec)) for b in beta]
    n0 = M.n0_of(idx)
    H = [level0(K.imported(beta, per), sz, idx, faces, per)]
    for l in range(1, len(M.level_dims(n0))):
        mask, wraps = P.level_state(n0, l, faces, per)
        H.append(coarsen(H[-1], mask, wraps))
    return H


def count_bad(H):
    """what the build counts on the device: the weights and diagonals of levels >= 1 that are not finite and positive, but for the stored
    zeros of the faces without a link"""
    def ok(a):
        return np.isfinite(a) & (a > 0)
    n = 0
    for l, L in enumerate(H):
        if l == 0:
            continue
        n += int((~ok(L.D)).sum())
        for d in range(3):
            bad = ~ok(L.W[d])
            for side, sel in ((0, 0), (1, -1)):
                if L.cut[2 * d + side]:
                    _take(bad, d, sel)[...] = False
            n += int(bad.sum())
    return n


def padded(u, L):
    """u with one shell: zeros, the mirror on the level's mirrored faces, the wrap in its wrapped directions (edges are not read)"""
    p = np.pad(u, 1)
    core = (slice(1, -1),) * 2
    for d in range(3):
        q = np.moveaxis(p, _NORMAL[d], 0)
        if L.wraps[d]:
            q[0][core] = q[-2][core]
            q[-1][core] = q[1][core]
        else:
            if L.mirrors[2 * d]:
                q[0][core] = q[1][core]
            if L.mirrors[2 * d + 1]:
                q[-1][core] = q[-2][core]
    return p


def ss(u, L):
    X, Y, Z = L.W
    p = padded(u, L)
    c = slice(1, -1)
    return (X[:, 1:, :] * p[c, 2:, c] + X[:, :-1, :] * p[c, :-2, c] + Y[1:] * p[2:, c, c] + Y[:-1] * p[:-2, c, c]
            + Z[:, :, 1:] * p[c, c, 2:] + Z[:, :, :-1] * p[c, c, :-2])  # left to right


def sweep(u, b, L, omg):
    """one relaxed Jacobi sweep of the level (u None: the from-zero form, which reads only b and D)"""
    R = b.dtype.type
    if u is None:
        dp = ((R(0) - b) / L.D - R(0)) * R(omg)
        return R(0) + dp
    dp = ((ss(u, L) - b) / L.D - u) * R(omg)
    return u + dp


def residual(x, b, L):
    return b - (ss(x, L) - L.D * x)


def restrict(x, b, L):
    return M._pair(M._pair(M._pair(residual(x, b, L), 2), 1), 0)


def colour_sweep(u, b, L, omg, c):
    """one colour sweep in place: the update of every point from the array as it is before the sweep, kept at the points of colour c"""
    if u is None:
        u = np.zeros_like(b)
    return np.where(RB.colour(b.shape) == c, sweep(u, b, L, omg), u)


def pair(x, b, L, omg, kind, post):
    """two smoothing iterations (x None: from zero): mg relaxed Jacobi sweeps, mgrb forward (colour 0, 1) or backward (post) iterations"""
    for _ in range(2):
        if kind == "mg":
            x = sweep(x, b, L, omg)
        else:
            first = 1 if post else 0
            x = colour_sweep(colour_sweep(x, b, L, omg, first), b, L, omg, 1 - first)
    return x


def vcycle(b, l, H, omg, kind):
    """x = V_l(b): mg_walk's order"""
    if l == len(H) - 1:
        x = pair(None, b, H[l], omg, kind, False)
        x = pair(x, b, H[l], omg, kind, False)
        for _ in range(2):
            x = pair(x, b, H[l], omg, kind, True)
        return x
    x = pair(None, b, H[l], omg, kind, False)
    xc = vcycle(restrict(x, b, H[l]), l + 1, H, omg, kind)
    return pair(M.prolong(x, xc), b, H[l], omg, kind, True)


def tail(b, t, H, omg, kind):
    """x = V_t(b) as the one-workgroup tail kernel states it: loops down and up over the levels t .. coarsest, no recursion"""
    n = len(H)
    bs, xs = {t: b}, {}
    for l in range(t, n - 1):
        xs[l] = pair(None, bs[l], H[l], omg, kind, False)
        bs[l + 1] = restrict(xs[l], bs[l], H[l])
    x = None
    for s in range(4):
        x = pair(x, bs[n - 1], H[n - 1], omg, kind, s >= 2)
    xs[n - 1] = x
    for l in range(n - 2, t - 1, -1):
        xs[l] = pair(M.prolong(xs[l], xs[l + 1]), bs[l], H[l], omg, kind, True)
    return xs[t]


def apply(kind, H, r, sz, idx, omg):
    """z = M_beta^-1 r on full S3D arrays (the cells outside the inner box stay zero)"""
    R = r.dtype.type
    ins = M.inner(sz, idx)
    z = np.zeros_like(r)
    z[ins] = vcycle(np.ascontiguousarray(r[ins]), 0, H, R(omg), kind)
    return z


class CZ(K.CZ):
    """coef_parity.CZ whose Preconditioner is the coefficient cycle while H is set (None: the parent's scaled one)"""
    H = None

    def Preconditioner(self, xx, bb, pc):
        if self.H is None or not (self._mg or self._mgrb):
            return super().Preconditioner(xx, bb, pc)
        xx[...] = apply("mgrb" if self._mgrb else "mg", self.H, bb, self.size, self.idx, self.ac1)
        self.cycles += 1


def solver(gsz, coef, prec, state, beta, perturb=0, on=True):
    faces, per, closed = state
    assert P.solvable(faces, per, closed)
    k = K.Kernels("oracle", prec)
    k.faces, k.per = tuple(faces), tuple(per)
    cz = CZ(k, wide=False, dots="exact", perturb=perturb)
    cz.closed = bool(closed)
    cz.setup(list(gsz), coef)
    k.user = True
    k.B = K.imported(beta, per)
    cz.s = K.scaling(k.B, cz.size, cz.idx)
    if on:
        cz.H = hierarchy(beta, gsz, state)
    return cz, k


def run(gsz, pc, coef, prec, state, itr_max, b, p, beta, eps=None, perturb=0, on=True):
    """coef_parity.run with the coefficient cycle as the preconditioner of mg | mgrb (on=False: that run itself)"""
    import closed_parity as C
    cz, k = solver(gsz, coef, prec, state, beta, perturb, on)
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
    that the runs with every sum at either edge give its bits (coef_parity.premise_f32)"""
    r0 = run(gsz, pc, coef, "f32", state, itr_max, b, p, beta, eps=eps)
    f = CP.flips(r0, "f32")
    assert not f, f"dots within their summation bound of a float boundary {f[:4]}"
    if state[2]:
        for q in (-1, 1):
            rq = run(gsz, pc, coef, "f32", state, itr_max, b, p, beta, eps=eps, perturb=q)
            assert rq.itr == r0.itr and rq.history == r0.history, q
            assert rq.P.tobytes() == r0.P.tobytes() and rq.B.tobytes() == r0.B.tobytes(), q
    return r0


def level_operator(L):
    """the level's operator as a dense matrix in double, C order [I, J, K]: A x = -(residual of x with b = 0)"""
    nj, ni, nk = L.shape
    n = ni * nj * nk
    A = np.zeros((n, n))
    Ld = Level([w.astype(np.float64) for w in L.W], L.mirrors, L.wraps)
    for q in range(n):
        e = np.zeros(n)
        e[q] = 1.0
        x = np.ascontiguousarray(e.reshape((ni, nj, nk)).transpose(1, 0, 2))
        A[:, q] = -np.ascontiguousarray(residual(x, np.zeros_like(x), Ld).transpose(1, 0, 2)).ravel()
    return A


def aggregation(fine_shape):
    """P of one coarsening step as a dense 0 / 1 matrix, (fine points) x (coarse points), both C order [i, j, k]; shapes are [j, i, k]"""
    nj, ni, nk = fine_shape
    cj, ci, ck = [(v + 1) // 2 for v in fine_shape]
    Pm = np.zeros((ni * nj * nk, ci * cj * ck))
    for i in range(ni):
        for j in range(nj):
            for k in range(nk):
                Pm[(i * nj + j) * nk + k, ((i >> 1) * cj + (j >> 1)) * ck + (k >> 1)] = 1.0
    return Pm


# ---- the GPU cases (tests/test_gpu_coefmg.py), chosen on the CPU (tests/test_coefmg_oracle.py: the FP32 premise, the FP64 envelope)
def case(gsz, pc, coef, prec, Kit, state, field, seed=0):
    return dict(gsz=tuple(gsz), pc=pc, coef=coef, prec=prec, K=Kit, state=state, field=field, seed=seed,
                id=f"pcg_{pc}_{'x'.join(map(str, gsz))}_{prec}_{state}_{field}_K{Kit}")


PCG_CASES = [
    case((9, 7, 12), "mg", 0.8, "f32", 3, "channel", "random"),
    case((9, 7, 12), "mgrb", 1.2, "f64", 3, "closed", "bubble1000"),
    case((9, 7, 12), "mgrb", 1.2, "f32", 3, "inflow", "random"),
    case((33, 47, 61), "mg", 0.8, "f64", 4, "inflow", "bubble1000"),
    case((33, 47, 61), "mgrb", 1.2, "f32", 4, "dirichlet", "bubble1000"),
    case((33, 47, 61), "mg", 0.8, "f32", 3, "closed", "random"),
    # (FP32, bit for bit.  The FP64 run of this case was measured on the GPU at most 2.8e-15 from the restatement, the envelope reaching
    # 7.8e-11, but at 2 of its 2.1 million points the pointwise envelope is one ulp of the field's maximum and the deviation 6.7e-16 is
    # 2.7 x the bar there: the pointwise bar is no premise that the CPU can establish at this size)
    case((40, 40, 1100), "mgrb", 1.2, "f32", 2, "channel", "random"),
    case((40, 40, 1100), "mg", 0.8, "f32", 2, "dirichlet", "bubble1000"),
]


def case_problem(c):
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    return b, p, FIELDS[c["field"]](c["gsz"], c["prec"])


def case_run(c, perturb=0):
    b, p, beta = case_problem(c)
    return run(c["gsz"], c["pc"], c["coef"], c["prec"], K.STATES[c["state"]], c["K"], b, p, beta, eps=1e-30, perturb=perturb)


# ---- iterations to coef_parity.COUNT_EPS on the seeded problem at coef_parity.COUNT_BOX, FP64, Dirichlet faces, ItrMax 300, with the
# coefficient cycle (tests/coefmg_measured.py; tests/test_coefmg_oracle.py re-measures them and checks them against the scaled counts)
COUNT_BOX, COUNT_EPS, COUNT_RUNS = K.COUNT_BOX, K.COUNT_EPS, K.COUNT_RUNS
