"""The closed box for pcg, restated on the oracle (importable without a GPU): what tests/test_closed_oracle.py checks on the
CPU and tests/test_gpu_closed.py compares the GPU driver with.

All six faces are zero-flux faces.  The operator N is then singular, its null space the constants, and three projections keep the solve
well posed (`CZ.PCG` below is neumann_parity.CZ's loop with them; with `closed` off it IS that loop):

1. start: r = b - N x, m0 = R(sum r / npts), r <- r - m0; the pass that writes r' returns sum r' (the first lagged mean) and sum r'^2
   (`none`'s first rho);
2. every update: r_new = R(R(R(-alpha q) + r) - m), m = R(sum r / npts) of the residual as the update before wrote it;
3. end: mx = R(sum x / npts), x <- x - mx, then the mirror.

The right-hand side is projected the same way when the mode is switched on and after every set_rhs (`project`).

The sums.  A dot product here follows cg_parity's recipe: the correctly rounded sum S of the per-point terms and R(S + perturb * B), B the
bound on how far any order of double summation lies from S, (n - 1) u sum|t| to first order.  A mean is R((S + perturb * B) / npts), and the
lagged S is rounding drift: it is small against sum|r|, so under the any-order bound the two edges nearly always round to different REALs
and the FP32 bar of bit equality would have no premise.  The kernels do not sum in any order, though: a term passes through at most d
additions, and for such a summation the error is at most gamma_d sum|t| (Higham, Accuracy and Stability of Numerical Algorithms, §4.2).
d for shift_sums_k and cg_update_k: a thread's own chain, V ceil(nplanes / gridDim.y) <= 4 where every plane has its own row of
workgroups (`chain` below computes it for a box; every box of the tests has 4 at most); the workgroup's reduction (block_sum<256>), 6
shuffle levels inside a wave and thread 0's chain over the four waves (0.0 + w0 + ... + w3), 10; the last workgroup's chain over the
partials, ceil(nblk / 256) <= 17 for the <= 4096 + gx workgroups of a launch; its reduction, 10 again; an all-reduce over at most 8
ranks, 7.  That is 48 (`depth` below); SUM_DEPTH = 64 leaves room.  B = gamma_64 sum|t| is the bound of the sums of this file.

FP32 premise (`premise_f32`): r_new is monotone in m and m is monotone in S, so where the runs with every sum at -B and at +B give the bits
of the unperturbed run -- fields, history, the means of b and x -- every summation within the bound does.  FP64: the envelope of those runs.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cg_parity as CP  # noqa: E402
import mg_parity as M  # noqa: E402
import neumann_parity as N  # noqa: E402
import problem_parity as PP  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

SIX = (1, 1, 1, 1, 1, 1)
SUM_DEPTH = 64
BOXES = [(9, 7, 12), (33, 47, 61), (6, 5, 1030), (3, 40, 40), (32, 36, 40), (64, 64, 64)]


def chain(gsz, prec):
    """the longest chain of additions in one thread of shift_sums_k / cg_update_k on the single-domain box: V ceil(nplanes / gridDim.y)"""
    V = 4 if prec == "f32" else 2
    nkp = gsz[2] + 2 * O.GUIDE
    R = -(-nkp // V)
    gx = -(-((gsz[0] - 2) * R) // 256)
    nplanes = gsz[1] - 2
    gy = max(1, min(nplanes, 4096 // gx))
    return V * -(-nplanes // gy)


def depth(gsz, prec):
    """the additions a term passes through at most in a sum of shift_sums_k / cg_update_k (this file's docstring)"""
    return chain(gsz, prec) + 10 + 17 + 10 + 7


def sum_bound(t):
    """(S, B) of the terms t (doubles): the correctly rounded sum and gamma_d sum|t|, d = SUM_DEPTH"""
    t = np.asarray(t, dtype=np.float64).ravel()
    u = 2.0 ** -53
    g = SUM_DEPTH * u / (1.0 - SUM_DEPTH * u)
    return math.fsum(t), g * math.fsum(np.abs(t))


def mean_of(t, npts, R, perturb=0):
    """m = R((S + perturb B) / npts): double division, one rounding; (m, S, B)"""
    S, B = sum_bound(t)
    return R((S + perturb * B) / npts), S, B


def mean_tol(m, B, npts):
    """how far a mean made from any sum within B of the exact one lies from m: B / npts and the rounding of either (FP64's bar; in FP32
    the premise makes it zero)"""
    return B / npts + float(np.spacing(np.abs(m)))


def project(a, sz, idx, perturb=0, tol=False):
    """a <- a - mean(a) over the inner box of the padded array a, in place; returns m (the REAL), with tol also mean_tol of it"""
    ins = M.inner(sz, idx)
    R = a.dtype.type
    m, _, B = mean_of(a[ins], a[ins].size, R, perturb)
    a[ins] = a[ins] - m
    return (m, mean_tol(m, B, a[ins].size)) if tol else m


class CZ(N.CZ):
    """neumann_parity.CZ whose PCG makes the three projections while `closed` is set (k: a neumann_parity.Kernels with six faces)"""

    closed = True

    def PCG(self, X, B, ItrMax, pc):
        if not self.closed:
            return super().PCG(X, B, ItrMax, pc)
        assert pc in ("none", "jacobi", "mg", "mgrb") and self.dots == "exact"
        self._mgrb, self._mg, self.cycles = pc == "mgrb", pc in ("mg", "mgrb"), 0
        self.sum_log, self.means = [], [None, None, None]
        k, R, sz, idx = self.k, self.R, self.size, self.idx
        ins = M.inner(sz, idx)
        n = X[ins].size
        mu = (n - 1) * 2.0 ** -53
        gamma = mu / (1.0 - mu)
        itr = 1

        def dot2(x, y, which):
            t = np.multiply(x[ins], y[ins], dtype=R).astype(np.float64).ravel()
            S = math.fsum(t)
            Bd = gamma * math.fsum(np.abs(t))
            self.dot_log.append((itr, which, S, Bd, n))
            return R(S + self.perturb * Bd)

        def mean(x, which):
            m, S, Bd = mean_of(x[ins], n, R, self.perturb)
            self.sum_log.append((itr, which, S, Bd, n))
            self.last_tol = mean_tol(m, Bd, n)
            return m

        a = {name: k.alloc(sz) for name in ("r", "z", "p", "q")}
        r = a["r"]
        res, rr, rho_old = 0.0, None, None
        k.blas_calc_rk(r, X, B, sz, idx, self.cf)
        m0 = mean(r, "r0")
        r[ins] = r[ins] - m0
        self.means[1] = m0
        m = mean(r, "r0'")
        if pc == "none":
            rr = dot2(r, r, "rho")
        while itr <= ItrMax:
            if pc != "none":
                k.blas_clear(a["z"], sz)
                self.Preconditioner(a["z"], r, "jacobi")
                z = a["z"]
                rho = dot2(r, z, "rho")
            else:
                z = r
                rho = rr
            if abs(float(rho)) < O.FLT_MIN:
                itr = 0
                break
            if itr == 1:
                k.blas_copy(a["p"], z, sz)
            else:
                k.blas_triad(a["p"], a["p"], z, R(rho / rho_old), sz, idx)
            k.blas_calc_ax(a["q"], a["p"], sz, idx, self.cf)
            alpha = R(rho / dot2(a["p"], a["q"], "p.q"))
            k.blas_triad(X, a["p"], X, alpha, sz, idx)
            k.blas_triad(r, a["q"], r, R(-alpha), sz, idx)
            r[ins] = r[ins] - m
            m = mean(r, "r")
            rr = dot2(r, r, "r.r")
            res = math.sqrt(float(rr) * self.res_normal)
            self.history.append((itr, res))
            if res < self.eps:
                break
            rho_old = rho
            itr += 1
        itr = min(itr, ItrMax)
        mx = mean(X, "x")
        X[ins] = X[ins] - mx
        self.means[2], self.tol_x = mx, self.last_tol
        return itr, res


def solver(gsz, coef, prec, perturb=0, closed=True, faces=SIX):
    k = N.Kernels("oracle", prec)
    k.faces = tuple(faces)
    cz = CZ(k, wide=False, dots="exact", perturb=perturb)
    cz.closed = closed
    cz.setup(list(gsz), coef)
    k.user = True
    return cz, k


def run(gsz, pc, coef, prec, itr_max, b, p, eps=None, perturb=0, closed=True, faces=SIX):
    """`pcg itr_max coef pc` in the closed box on the problem (b, p) [i, j, k]: b projected as set_rhs does, then the solve.  O.Result with
    P (mirrors in place), means = [m_b, m_0, m_x], sum_log.  closed=False with a mask of fewer faces: neumann_parity.run"""
    cz, k = solver(gsz, coef, prec, perturb, closed, faces)
    cz.P, cz.RHS = PP.pad(p), PP.pad(b)
    mb, tol_b = project(cz.RHS, cz.size, cz.idx, perturb, tol=True) if closed else (None, None)
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
        out.mean_tol = [tol_b, None, cz.tol_x]  # (the mean of the initial residual is rounding drift: no bar)
        out.sum_log = cz.sum_log
        out.B = cz.RHS
    return out


def envelope_f64(gsz, pc, coef, itr_max, b, p, eps=None):
    r = {q: run(gsz, pc, coef, "f64", itr_max, b, p, eps=eps, perturb=q) for q in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr, [r[q].itr for q in (-1, 0, 1)]
    P0, h0 = r[0].P, np.array([v for _, v in r[0].history])
    E = np.maximum(np.abs(r[1].P - P0), np.abs(r[-1].P - P0))
    Eh = np.maximum(np.abs(np.array([v for _, v in r[1].history]) - h0), np.abs(np.array([v for _, v in r[-1].history]) - h0))
    return r[0], E, Eh


def premise_f32(gsz, pc, coef, itr_max, b, p, eps=None):
    """the unperturbed FP32 run, after asserting that no dot lies within its bound of a rounding boundary and that the runs with every sum
    and dot at either edge give its bits"""
    r0 = run(gsz, pc, coef, "f32", itr_max, b, p, eps=eps)
    f = CP.flips(r0, "f32")
    assert not f, f"dots within their summation bound of a float boundary {f[:4]}"
    for q in (-1, 1):
        rq = run(gsz, pc, coef, "f32", itr_max, b, p, eps=eps, perturb=q)
        assert rq.itr == r0.itr and rq.history == r0.history, q
        assert rq.P.tobytes() == r0.P.tobytes() and rq.B.tobytes() == r0.B.tobytes(), q
        # (m_0 and the lagged means are rounding drift, sums that cancel: their own bits do move inside the bound; what they are subtracted
        # from does not, which is what the lines above assert)
        assert float(rq.means[0]) == float(r0.means[0]) and float(rq.means[2]) == float(r0.means[2]), (q, rq.means, r0.means)
    return r0


def mean_bound(mx, xmax, R):
    """|mean of the returned field x' = x - mx| <= this (mx: the mean removed, xmax: max|x'|).  mx = R(S~ / npts) with S~ within
    B = gamma_64 sum|x| of the exact sum S, so |S / npts - mx| <= ulp(mx) / 2 + gamma_64 mean|x|, and mean|x| <= |mx| + xmax; every
    subtraction rounds by at most ulp(xmax) / 2, and so does their mean.  Nothing in it grows with npts: the depth of the kernels' summation
    does not (closed_parity's docstring), and the mean of the per-cell roundings is bounded by the largest of them."""
    u = 2.0 ** -53
    g = SUM_DEPTH * u / (1.0 - SUM_DEPTH * u)
    return 0.5 * float(np.spacing(R(abs(mx)))) + 0.5 * float(np.spacing(R(xmax))) + g * (abs(float(mx)) + float(xmax))


# ---- the GPU cases (tests/test_gpu_closed.py); the seeds are chosen on the CPU so that the FP32 premise holds (tests/test_closed_oracle.py)
def case(gsz, pc, coef, prec, K, seed=0):
    return dict(gsz=tuple(gsz), pc=pc, coef=coef, prec=prec, K=K, seed=seed, id=f"pcg_{pc}_{'x'.join(map(str, gsz))}_{prec}_closed_K{K}")


CASES = [
    case((9, 7, 12), "none", 0.8, "f32", 4),
    case((9, 7, 12), "jacobi", 0.8, "f64", 4),
    case((9, 7, 12), "mg", 0.8, "f32", 3),
    case((9, 7, 12), "mgrb", 1.2, "f64", 3),
    case((33, 47, 61), "none", 0.8, "f64", 5),
    case((33, 47, 61), "jacobi", 0.8, "f32", 4),
    case((33, 47, 61), "mg", 0.8, "f64", 4),
    case((33, 47, 61), "mgrb", 1.0, "f32", 4, seed=2),  # (seeds 0 and 1: an update's bits move inside the bound of its lagged mean)
]


def case_run(c, perturb=0):
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    return run(c["gsz"], c["pc"], c["coef"], c["prec"], c["K"], b, p, eps=1e-30, perturb=perturb)


# iterations to eps 1e-5 on the seeded (incompatible) problem at 33 x 47 x 61, FP64, ItrMax 300 (tests/test_closed_oracle.py records them)
COUNT_BOX = (33, 47, 61)
COUNT_RUNS = [("none", 0.8), ("jacobi", 0.8), ("mg", 0.8), ("mgrb", 1.2)]
COUNTS = {("none", 0.8): 150, ("jacobi", 0.8): 40, ("mg", 0.8): 7, ("mgrb", 1.2): 4}

# decomposed runs on the LOCAL transport (case, division): solved to eps 1e-5 within ItrMax 100
DECOMP = [(dict(gsz=(32, 36, 40), prec="f32", pc="jacobi", coef=0.8, id="jacobi_32x36x40_f32_2x2x2"), (2, 2, 2)),
          (dict(gsz=(32, 36, 40), prec="f64", pc="mg", coef=0.8, id="mg_32x36x40_f64_2x1x2"), (2, 1, 2))]


def manufactured(gsz):
    """(u, b) in FP64: problem_parity.manufactured's smooth u less its mean over the inner box, mirrored onto the six faces, and b = N u by
    the oracle's blas_calc_ax on the mirrored field (zero sum up to rounding; set_rhs projects it)"""
    k = N.Kernels("oracle", "f64")
    k.faces = SIX
    u, _, _ = PP.manufactured(gsz)
    u = u.copy()
    u[1:-1, 1:-1, 1:-1] -= math.fsum(u[1:-1, 1:-1, 1:-1].ravel()) / u[1:-1, 1:-1, 1:-1].size
    sz = list(gsz)
    idx, _ = O.range_inner_index(sz, [-1] * 6)
    U = PP.pad(u)
    N.mirror(U, sz, idx, SIX)
    AU = k.alloc(sz)
    k.blas_calc_ax(AU, U, sz, idx, np.array([1, 1, 1, 1, 1, 1, 6], dtype=np.float64))
    return PP.unpad(U), PP.unpad(AU)


def refine(b, p, tol=1e-10, max_outer=20, inner_eps=None, inner=("mgrb", 1.2)):
    """neumann_parity.refine in the closed box: the FP64 side holds b projected (set_rhs with the mode on), every inner FP32 solve projects
    the scaled residual it is handed and returns a correction of zero mean.  (outer steps or 0, history, p, ratios)"""
    import refine_parity as RP
    inner_eps = RP.INNER_EPS if inner_eps is None else inner_eps
    gsz = list(p.shape)
    k = N.Kernels("oracle", "f64")
    k.faces = SIX
    idx, _ = O.range_inner_index(gsz, [-1] * 6)
    cf = np.array([1, 1, 1, 1, 1, 1, 6], dtype=np.float64)
    B = PP.pad(b.astype(np.float64))
    project(B, gsz, idx)

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
        o = run(gsz, inner[0], inner[1], "f32", 1000, r32, np.zeros(gsz, dtype=np.float32), eps=inner_eps)
        its = o.itr
        p = RP.add(p, PP.unpad(o.P), 1.0 / scale)
        step += 1
