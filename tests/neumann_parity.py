"""Zero-flux (Neumann) faces for pcg, restated on the oracle (importable without a GPU): what
tests/test_neumann_oracle.py checks on the CPU and tests/test_gpu_neumann.py compares the GPU driver with.

A mask is six flags in the order X-, X+, Y-, Y+, Z-, Z+ (the order of nID); at least one face stays Dirichlet.  Two rules:

* level 0 keeps the unit-coefficient kernels and D = 6.  On a Neumann face the face layer is the mirror of the first inner layer,
  p(1, j, k) = p(2, j, k) and p(size, j, k) = p(size-1, j, k) over the inner box, and it is re-made before every kernel that reads the
  field's neighbours: `Kernels` below is problem_parity.Kernels whose jacobi, psor2sma_core, blas_calc_ax and blas_calc_rk mirror their input
  first.  The restriction of level 0 reads the same layer (`restrict0`; mg_parity.restrict pads with zeros, which is the same thing without
  a mask);
* levels >= 1 need no mirror (the correction is zero outside the box, the absent link is W * 0); only the Galerkin diagonal changes,
  D = Wx cx + Wy cy + Wz cz with c = 2 less one per Neumann face the point lies on.  `masked` exchanges mg_parity.weights for that (the
  cycles of mg_parity and mgrb_parity look the function up in that module at every call), as mgrb_parity.envelope_f64 exchanges
  mg_parity.oracle.

The solver class is mgrb_parity.CZ (PCG with none | jacobi | mg | mgrb, exact dots) with the V-cycles routed through `apply` below.
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_parity as M  # noqa: E402
import mgrb_parity as RB  # noqa: E402
import problem_parity as PP  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

NONE = (0, 0, 0, 0, 0, 0)
Z_BOTH = (0, 0, 0, 0, 1, 1)
X_PLUS = (0, 1, 0, 0, 0, 0)
X_MINUS = (1, 0, 0, 0, 0, 0)
X_BOTH = (1, 1, 0, 0, 0, 0)
MIXED = (0, 1, 1, 0, 0, 1)       # X+ Y- Z+
FIVE = (1, 1, 1, 1, 1, 0)        # every face but Z+
MINUS3 = (1, 0, 1, 0, 1, 0)
MASKS = {"none": NONE, "z": Z_BOTH, "xp": X_PLUS, "five": FIVE}

_UNMASKED_WEIGHTS = M.weights


def bits(faces):
    return sum(1 << f for f in range(6) if faces[f])


def mirror(p, sz, idx, faces):
    """the Neumann face layers of the padded array p [j + 2, i + 2, k + 2] from its first inner layers, in place; only faces that are physical
    faces of the brick (idx starts at 2 / ends at size - 1 there)"""
    js, is_, ks = M.inner(sz, idx)
    if faces[0] and idx[0] == 2:
        p[js, is_.start - 1, ks] = p[js, is_.start, ks]
    if faces[1] and idx[1] == sz[0] - 1:
        p[js, is_.stop, ks] = p[js, is_.stop - 1, ks]
    if faces[2] and idx[2] == 2:
        p[js.start - 1, is_, ks] = p[js.start, is_, ks]
    if faces[3] and idx[3] == sz[1] - 1:
        p[js.stop, is_, ks] = p[js.stop - 1, is_, ks]
    if faces[4] and idx[4] == 2:
        p[js, is_, ks.start - 1] = p[js, is_, ks.start]
    if faces[5] and idx[5] == sz[2] - 1:
        p[js, is_, ks.stop] = p[js, is_, ks.stop - 1]
    return p


class Kernels(PP.Kernels):
    """problem_parity.Kernels whose neighbour-reading kernels mirror their input first"""
    faces = NONE

    def mirror(self, p, sz, idx):
        if any(self.faces):
            mirror(p, sz, idx, self.faces)

    def jacobi(self, p, sz, idx, *a, **kw):
        self.mirror(p, sz, idx)
        return super().jacobi(p, sz, idx, *a, **kw)

    def psor2sma_core(self, p, sz, idx, *a, **kw):
        self.mirror(p, sz, idx)
        return super().psor2sma_core(p, sz, idx, *a, **kw)

    def blas_calc_ax(self, ap, p, sz, idx, cf):
        self.mirror(p, sz, idx)
        return super().blas_calc_ax(ap, p, sz, idx, cf)

    def blas_calc_rk(self, r, p, b, sz, idx, cf):
        self.mirror(p, sz, idx)
        return super().blas_calc_rk(r, p, b, sz, idx, cf)


def links(n, minus, plus):
    """c(I) = 2 - [I first and the - face Neumann] - [I last and the + face Neumann], I = 0 .. n-1"""
    c = np.full(n, 2, dtype=np.int64)
    if minus:
        c[0] -= 1
    if plus:
        c[-1] -= 1
    return c


def weights(n0, level, R, faces):
    """mg_parity.weights with the masked diagonal on levels >= 1 (level 0: 1 and 6 whatever the mask, the mirror carries the condition)"""
    wx, wy, wz, d = _UNMASKED_WEIGHTS(n0, level, R)
    if level == 0 or not any(faces):
        return wx, wy, wz, d
    ni, nj, nk = M.level_dims(n0)[level]
    cx, cy, cz = links(ni, faces[0], faces[1]), links(nj, faces[2], faces[3]), links(nk, faces[4], faces[5])
    # small integers: exact in either precision (the products are taken in int64)
    di = (wx.astype(np.int64) * cx[None, :, None] + wy.astype(np.int64) * cy[:, None, None] + wz.astype(np.int64) * cz[None, None, :])
    return wx, wy, wz, di.astype(R)


@contextlib.contextmanager
def masked(faces):
    """inside: mg_parity's and mgrb_parity's coarse cycles take the masked diagonal"""
    keep = M.weights
    M.weights = lambda n0, level, R: weights(n0, level, R, faces)
    try:
        yield
    finally:
        M.weights = keep


def restrict0(z, r, sz, idx):
    """b_1 = level 0's residual b - (ss - 6 x) summed over the children, the neighbours read from the padded array z itself (its face
    layers: zeros on Dirichlet faces, the mirror on Neumann ones); the bits of mg_parity.restrict where those layers are zero"""
    R = z.dtype.type
    js, is_, ks = M.inner(sz, idx)

    def sh(dj, di, dk):
        return z[js.start + dj:js.stop + dj, is_.start + di:is_.stop + di, ks.start + dk:ks.stop + dk]

    ss = sh(0, 1, 0) + sh(0, -1, 0) + sh(1, 0, 0) + sh(-1, 0, 0) + sh(0, 0, 1) + sh(0, 0, -1)  # c1 .. c6, every weight 1
    res = r[js, is_, ks] - (ss - R(6) * z[js, is_, ks])
    return M._pair(M._pair(M._pair(res, 2), 1), 0)


def apply(kind, k, r, sz, idx, omg, faces):
    """z = V_0(r) of `mg` | `mgrb` on full S3D arrays with the Neumann faces `faces`: level 0 through the oracle's kernels k (a `Kernels` of
    this file with k.faces = faces), the coarse levels mg_parity / mgrb_parity with the masked diagonal"""
    assert tuple(k.faces) == tuple(faces)
    R = k.real
    cf = np.array([1, 1, 1, 1, 1, 1, 6], dtype=R)
    n0 = M.n0_of(idx)
    ins = M.inner(sz, idx)
    z, wk2 = k.alloc(sz), k.alloc(sz)

    def pair(post):
        if kind == "mg":
            for _ in range(2):
                k.jacobi(z, sz, idx, cf, R(omg), r, wk2)
        else:
            for _ in range(2):
                RB.fine_iteration(k, z, r, sz, idx, omg, post)

    with masked(faces):
        if len(M.level_dims(n0)) == 1:
            for s in range(4):
                pair(s >= 2)
            return z
        pair(False)
        k.mirror(z, sz, idx)
        cycle = M.vcycle if kind == "mg" else RB.vcycle
        xc = cycle(restrict0(z, r, sz, idx), 1, n0, R(omg))
        z[ins] = M.prolong(z[ins], xc)
        pair(True)
    return z


class CZ(RB.CZ):
    """mgrb_parity.CZ whose V-cycles are those of this file (k: a `Kernels` of this file)"""

    def Preconditioner(self, xx, bb, pc):
        if not (self._mg or self._mgrb):
            return super().Preconditioner(xx, bb, pc)  # none: never called; jacobi: the 8 sweeps, each mirroring its input
        xx[...] = apply("mgrb" if self._mgrb else "mg", self.k, bb, self.size, self.idx, self.ac1, self.k.faces)
        self.cycles += 1


def solver(gsz, coef, prec, faces, perturb=0):
    """(cz, k): the set-up solver object for a caller's problem with the mask"""
    k = Kernels("oracle", prec)
    k.faces = tuple(faces)
    cz = CZ(k, wide=False, dots="exact", perturb=perturb)
    cz.setup(list(gsz), coef)
    k.user = True
    return cz, k


def run(gsz, pc, coef, prec, faces, itr_max, b, p, eps=None, perturb=0):
    """`pcg itr_max coef pc` on the problem (b, p) [i, j, k] with the mask: O.Result, P with the mirrors in place"""
    cz, k = solver(gsz, coef, prec, faces, perturb)
    cz.P, cz.RHS = PP.pad(p), PP.pad(b)
    k.mirror(cz.P, cz.size, cz.idx)
    if eps is not None:
        cz.eps = eps
    cz.cycles = 0
    itr, res = cz.PCG(cz.P, cz.RHS, itr_max, pc)
    k.mirror(cz.P, cz.size, cz.idx)
    out = O.Result(itr=itr, res=res, history=cz.history, P=cz.P, dot_log=cz.dot_log)
    out.cycles = cz.cycles
    return out


def envelope_f64(gsz, pc, coef, faces, itr_max, b, p, eps=None):
    """FP64: the unperturbed run and the envelope of the runs with every dot at either edge of its summation bound (field, history)"""
    r = {q: run(gsz, pc, coef, "f64", faces, itr_max, b, p, eps=eps, perturb=q) for q in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr, [r[q].itr for q in (-1, 0, 1)]
    P0, h0 = r[0].P, np.array([v for _, v in r[0].history])
    E = np.maximum(np.abs(r[1].P - P0), np.abs(r[-1].P - P0))
    Eh = np.maximum(np.abs(np.array([v for _, v in r[1].history]) - h0), np.abs(np.array([v for _, v in r[-1].history]) - h0))
    return r[0], E, Eh


def assembled(gsz, faces):
    """the zero-flux operator N as a dense matrix on the inner cells of a small box, C order [i, j, k]: 1 per neighbour that is an inner cell,
    and on the diagonal -6 plus one per neighbour across a Neumann face (a neighbour across a Dirichlet face contributes its value, which
    is not part of the matrix: the caller tests with zero Dirichlet values)"""
    n = [v - 2 for v in gsz]
    N = np.zeros((n[0] * n[1] * n[2],) * 2)
    at = lambda i, j, k: (i * n[1] + j) * n[2] + k  # noqa: E731
    for i in range(n[0]):
        for j in range(n[1]):
            for k in range(n[2]):
                q, c = at(i, j, k), (i, j, k)
                N[q, q] = -6.0
                for d in range(3):
                    for s in (-1, 1):
                        m = list(c)
                        m[d] += s
                        if 0 <= m[d] < n[d]:
                            N[q, at(*m)] = 1.0
                        elif faces[2 * d + (s > 0)]:
                            N[q, q] += 1.0
    return N


def manufactured(gsz, faces):
    """(u, b, p) in FP64: a smooth u on the inner cells, mirrored onto the Neumann faces (and kept on the Dirichlet ones), b = A u by the
    oracle's blas_calc_ax on the mirrored field, p = u on the faces and zero inside"""
    k = Kernels("oracle", "f64")
    k.faces = tuple(faces)
    u, _, _ = PP.manufactured(gsz)
    sz = list(gsz)
    idx, _ = O.range_inner_index(sz, [-1] * 6)
    U = PP.pad(u)
    mirror(U, sz, idx, faces)
    AU = k.alloc(sz)
    k.blas_calc_ax(AU, U, sz, idx, np.array([1, 1, 1, 1, 1, 1, 6], dtype=np.float64))
    u = PP.unpad(U)
    p = u.copy()
    p[1:-1, 1:-1, 1:-1] = 0.0
    return u, PP.unpad(AU), p


# ---- mixed-precision refinement with the mask (tests/refine_parity.refine with the mirrored residual and the masked inner solve)
def refine(b, p, faces, tol=1e-10, max_outer=20, inner_eps=None, inner=("mgrb", 1.2)):
    """(outer steps taken or 0, history [(outer, |r| / |r0|, inner iterations)], p, ratios)"""
    import refine_parity as RP
    inner_eps = RP.INNER_EPS if inner_eps is None else inner_eps
    gsz = list(p.shape)
    k = Kernels("oracle", "f64")
    k.faces = tuple(faces)
    idx, _ = O.range_inner_index(gsz, [-1] * 6)
    cf = np.array([1, 1, 1, 1, 1, 1, 6], dtype=np.float64)
    B = PP.pad(b.astype(np.float64))

    def residual(q):
        """r on the updated cells, 0 on the faces; q comes back with the mirrors in place"""
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
        o = run(gsz, inner[0], inner[1], "f32", faces, 1000, r32, np.zeros(gsz, dtype=np.float32), eps=inner_eps)
        its = o.itr
        p = RP.add(p, PP.unpad(o.P), 1.0 / scale)
        step += 1


# ---- the GPU cases (tests/test_gpu_neumann.py), chosen on the CPU (tests/test_neumann_oracle.py: FP32 premise of bit equality, iteration counts)
def case(gsz, pc, coef, prec, K, mask, seed=0):
    return dict(gsz=tuple(gsz), pc=pc, coef=coef, prec=prec, K=K, mask=mask, faces=MASKS[mask], seed=seed,
                id=f"pcg_{pc}_{'x'.join(map(str, gsz))}_{prec}_{mask}_K{K}")


PCG_CASES = [
    case((9, 7, 12), "none", 0.8, "f32", 4, "z"),
    case((9, 7, 12), "jacobi", 0.8, "f64", 4, "five"),
    case((9, 7, 12), "mg", 0.8, "f32", 3, "five"),
    case((9, 7, 12), "mgrb", 1.2, "f64", 3, "z"),
    case((33, 47, 61), "none", 0.8, "f64", 5, "five"),
    case((33, 47, 61), "jacobi", 0.8, "f32", 4, "z"),
    case((33, 47, 61), "mg", 0.8, "f64", 4, "z"),
    case((33, 47, 61), "mgrb", 1.0, "f32", 4, "five"),
]


# iterations to eps 1e-5 on the seeded problem at 33 x 47 x 61, FP64 (tests/test_neumann_oracle.py::test_oracle_iteration_counts records them)
COUNT_RUNS = [("none", 0.8), ("jacobi", 0.8), ("mg", 0.8), ("mgrb", 0.8), ("mgrb", 1.2)]
COUNTS = {("none", "none", 0.8): 81, ("none", "jacobi", 0.8): 21, ("none", "mg", 0.8): 9, ("none", "mgrb", 0.8): 7, ("none", "mgrb", 1.2): 5,
          ("five", "none", 0.8): 188, ("five", "jacobi", 0.8): 51, ("five", "mg", 0.8): 10, ("five", "mgrb", 0.8): 8, ("five", "mgrb", 1.2): 6}


def case_run(c, itr_max=None, perturb=0):
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    return run(c["gsz"], c["pc"], c["coef"], c["prec"], c["faces"], itr_max or c["K"], b, p, eps=1e-30, perturb=perturb)


# decomposed runs on the LOCAL transport (case, division, mask): solved to eps 1e-5 within ItrMax 100
DECOMP = [(dict(gsz=(32, 36, 40), prec="f32", pc="jacobi", coef=0.8, id="jacobi_32x36x40_f32_2x2x2"), (2, 2, 2), Z_BOTH),
          (dict(gsz=(32, 36, 40), prec="f64", pc="mg", coef=0.8, id="mg_32x36x40_f64_2x1x2"), (2, 1, 2), FIVE)]
