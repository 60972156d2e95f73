"""PCG restated on the oracle's kernels, its cases and its oracle-side premise (importable without a GPU).

`CZ.PCG` below is the loop of DESIGN.md "PCG (beyond the reference)" written with the C restatement's kernels (blas_calc_rk, the
preconditioner's Jacobi sweeps, blas_calc_ax, blas_triad, blas_copy) and the exact-dot recipe of oracle.cz_oracle.CZ.PBiCGSTAB: every dot
product takes the per-point products in REAL, sums them correctly rounded (math.fsum) to S and returns R(S + perturb * B), B the bound on
how far any order of double summation lies from S.  tests/bicg_parity.py explains what that buys:

* FP32: where no dot of the unperturbed run lies within its bound of a float rounding boundary, the GPU must equal the oracle bit for bit.
* FP64: the runs with every dot at -B / +B give the envelope E that bounds the GPU's distance from the unperturbed run.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import cz_oracle as O

ENVELOPE_MAX = 1e-8  # FP64: the envelope must stay below this (relative), or the case says nothing


class CZ(O.CZ):
    """oracle.cz_oracle.CZ with a PCG method (single domain, dots "exact" or the back-end's wide dots)."""

    def PCG(self, X, B, ItrMax, pc):
        assert pc in ("none", "jacobi")
        k, R, sz, idx = self.k, self.R, self.size, self.idx
        itr = 1
        if self.dots == "exact":
            g, (ist, ied, jst, jed, kst, ked) = O.GUIDE - 1, idx
            inner = (slice(jst + g, jed + g + 1), slice(ist + g, ied + g + 1), slice(kst + g, ked + g + 1))
            n = (ied - ist + 1) * (jed - jst + 1) * (ked - kst + 1)
            mu = (n - 1) * 2.0 ** -53
            gamma = mu / (1.0 - mu)

            def exact(t, which):
                t = t.astype(np.float64).ravel()  # exact: a REAL product is representable in double
                S = math.fsum(t)
                Bd = gamma * math.fsum(np.abs(t))
                self.dot_log.append((itr, which, S, Bd, n))
                return R(S + self.perturb * Bd)

            def dot2(x, y, which):
                return exact(np.multiply(x[inner], y[inner], dtype=R), which)  # REAL products, one rounding each, no FMA
        else:
            def dot2(x, y, which=None):
                w = np.zeros(1)
                k.blas_dot2(x, y, sz, idx, wide=w)
                return R(w[0])

        a = {name: k.alloc(sz) for name in ("r", "z", "p", "q")}
        res, rr, rho_old = 0.0, None, None
        k.blas_calc_rk(a["r"], X, B, sz, idx, self.cf)
        while itr <= ItrMax:  # at most ItrMax iterations
            if pc == "jacobi":
                k.blas_clear(a["z"], sz)
                self.Preconditioner(a["z"], a["r"], "jacobi")  # the 8 relaxed sweeps from zero
                z = a["z"]
                rho = dot2(a["r"], z, "rho")
            else:
                z = a["r"]  # M^-1 = I: z IS r
                rho = dot2(a["r"], a["r"], "rho") if itr == 1 else rr
            if abs(float(rho)) < O.FLT_MIN:  # breakdown
                itr = 0
                break
            if itr == 1:
                k.blas_copy(a["p"], z, sz)  # a copy, not z + 0*p
            else:
                beta = R(rho / rho_old)
                k.blas_triad(a["p"], a["p"], z, beta, sz, idx)  # p = R(beta*p) + z
            k.blas_calc_ax(a["q"], a["p"], sz, idx, self.cf)
            alpha = R(rho / dot2(a["p"], a["q"], "p.q"))
            k.blas_triad(X, a["p"], X, alpha, sz, idx)
            k.blas_triad(a["r"], a["q"], a["r"], R(-alpha), sz, idx)
            rr = dot2(a["r"], a["r"], "r.r")
            res = math.sqrt(float(rr) * self.res_normal)
            self.history.append((itr, res))
            if res < self.eps:
                break
            rho_old = rho
            itr += 1
        return min(itr, ItrMax), res


def run(gsz, itr_max, coef, pc="none", prec="f32", dots="exact", perturb=0, with_error=False, kind="oracle") -> O.Result:
    """``cz gsz pcg itr_max coef pc`` on the oracle"""
    cz = CZ(O.Kernels(kind, prec), wide=dots is None, dots=dots, perturb=perturb)
    cz.setup(gsz, coef)
    itr, res = cz.PCG(cz.P, cz.RHS, itr_max, pc)
    out = O.Result(itr=itr, res=res, history=cz.history, P=cz.P, dot_log=cz.dot_log)
    if with_error:
        out.errmax, out.errloc = cz.error_max()
    return out


def case(gsz, pc, coef, prec, K, every_k=True):
    return dict(gsz=tuple(gsz), solver="pcg", pc=pc, coef=coef, prec=prec, K=K, every_k=every_k,
                id=f"pcg_{pc}_{'x'.join(map(str, gsz))}_{prec}_K{K}")


# K iterations each (ItrMax = K: the loop makes at most ItrMax).  Chosen on the CPU with premise_f32 / envelope_f64 below
# (tests/test_cg_oracle.py::test_pcg_parity_premise).
CASES = [
    case((9, 7, 12), "none", 0.8, "f32", 4),
    case((9, 7, 12), "jacobi", 0.8, "f64", 4),
    case((33, 47, 61), "none", 0.8, "f32", 6),
    case((33, 47, 61), "jacobi", 0.8, "f32", 5),
    case((33, 47, 61), "none", 0.8, "f64", 6),
    case((33, 47, 61), "jacobi", 1.0, "f64", 5),
    case((64, 64, 64), "jacobi", 0.8, "f32", 5),
    case((64, 64, 64), "none", 0.8, "f64", 5),
    case((64, 64, 64), "jacobi", 0.8, "f64", 5),
    # k extent > 1 028 (FP64 rows beyond 1 020 elements: k-windowed preconditioner pass, several vectors per row in every kernel)
    case((40, 40, 1100), "jacobi", 0.8, "f64", 3),
    case((40, 40, 1100), "none", 0.8, "f32", 3),
    case((128, 128, 128), "jacobi", 0.8, "f32", 4, every_k=False),
]
# CZ_CG_FUSE=0 against the oracle
SWITCH_CASES = [c for c in CASES if c["gsz"] in ((33, 47, 61), (64, 64, 64))]
# decomposed runs (LOCAL transport, division (2, 1, 2))
DECOMP_CASES = [case((32, 36, 40), pc, 0.8, prec, 4, every_k=False) for pc in ("none", "jacobi") for prec in ("f32", "f64")]


def ks(c):
    """the iteration counts whose fields are compared"""
    return list(range(1, c["K"] + 1)) if c["every_k"] else [1, c["K"]]


def args(c, itr_max):
    return list(c["gsz"]) + ["pcg", itr_max, c["coef"], c["pc"]]


def oracle(c, itr_max, perturb=0):
    return run(c["gsz"], itr_max, c["coef"], c["pc"], prec=c["prec"], dots="exact", perturb=perturb)


def flips(r, prec):
    """dots of an exact-dot run whose two edges round to different REALs: (itr, which) of each"""
    R = np.float32 if prec == "f32" else np.float64
    return [(i, w) for (i, w, S, B, _) in r.dot_log if R(S - B) != R(S + B)]


def premise_f32(c, r0=None, perturbed=True):
    """FP32: no summation order can flip a rounding through iteration K.  Returns the unperturbed K-iteration run."""
    r0 = r0 or oracle(c, c["K"])
    f = flips(r0, "f32")
    assert not f, f"{c['id']}: premise fails (choose another case): dots within their summation bound of a float boundary {f[:4]}"
    if perturbed:
        for p in (-1, 1):
            rp = oracle(c, c["K"], p)
            assert rp.itr == r0.itr and rp.history == r0.history and rp.P.tobytes() == r0.P.tobytes(), (c["id"], p)
    return r0


def envelope_f64(c, itr_max):
    """FP64: the unperturbed run and the envelope of the two perturbed ones, field and history, at ItrMax = itr_max."""
    r = {p: oracle(c, itr_max, p) for p in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr, (c["id"], itr_max, [r[p].itr for p in (-1, 0, 1)])
    P0, h0 = r[0].P, np.array([v for _, v in r[0].history])
    E = np.maximum(np.abs(r[1].P - P0), np.abs(r[-1].P - P0))
    Eh = np.maximum(np.abs(np.array([v for _, v in r[1].history]) - h0), np.abs(np.array([v for _, v in r[-1].history]) - h0))
    rel = max(float(E.max() / np.abs(P0).max()), float((Eh / h0).max()) if len(h0) else 0.0)
    assert rel <= ENVELOPE_MAX, f"{c['id']}: FP64 envelope {rel:.2e} relative at ItrMax {itr_max}: too wide to test anything (choose a shorter K)"
    return r[0], E, Eh
