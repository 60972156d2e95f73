"""The V-cycle of `pcg ... mgrb` restated in numpy (importable without a GPU), and PCG with it on the oracle.

DESIGN.md §5.10.2 fixes the cycle down to the bit; it is the cycle of §5.10 (tests/mg_parity.py: levels, weights, restriction tree,
prolongation, coarsening stop) with the smoother exchanged:

* colour of a point: (I + J + K) & 1, (I, J, K) its 0-based indices in the level's inner box.  At level 0 that is the colouring of
  psor2sma_core with ofst = 0 on a single domain: its colour call `color` updates k = kst + mod(i + j + ofst + color, 2), ked, 2, and with
  ist = jst = kst the points of parity ofst + color;
* colour sweep: every point of one colour takes pn = pp + ((ss - bb)/D - pp) omg in place (points of one colour do not read each other);
* forward iteration F: colour 0, then colour 1.  Backward iteration B: colour 1, then colour 0;
* V_l(b): 2 F from zero, restrict, x_c = V_{l+1}, prolong, 2 B (the coarsest: 4 F from zero, then 4 B).  Level 0's iterations are the
  oracle's C psor2sma_core (ofst 0 for F, ofst 1 for B: colour calls 0, 1 each), the coarse levels this file's numpy.

B is the adjoint of F in the A-inner product, so the cycle is a symmetric preconditioner although no sweep of it is.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_parity as M  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

OMG_MAX = 1.2  # the largest coefficient offered (tests/test_mgrb_oracle.py: the smallest Ritz value of M A stays positive up to here)


def colour(shape):
    """(I + J + K) & 1 of every point of a level's inner box, shape (nj, ni, nk)"""
    j, i, k = np.indices(shape)
    return (i + j + k) & 1


def sweep(u, b, level, n0, omg, c):
    """one colour sweep of the level: the points of colour c take the relaxed update, the others stay (u None: from zero)"""
    if u is None:
        u = np.zeros_like(b)
    return np.where(colour(b.shape) == c, M.smooth(u, b, level, n0, omg), u)


def iteration(u, b, level, n0, omg, backward):
    """F (colour 0, 1) or B (colour 1, 0)"""
    first = 1 if backward else 0
    return sweep(sweep(u, b, level, n0, omg, first), b, level, n0, omg, 1 - first)


def vcycle(b, level, n0, omg):
    """x = V_l(b) in numpy at every level"""
    nlev = len(M.level_dims(n0))
    x = None
    if level == nlev - 1:
        for s in range(8):
            x = iteration(x, b, level, n0, omg, s >= 4)
        return x
    for _ in range(2):
        x = iteration(x, b, level, n0, omg, False)
    xc = vcycle(M.restrict(x, b, level, n0), level + 1, n0, omg)
    x = M.prolong(x, xc)
    for _ in range(2):
        x = iteration(x, b, level, n0, omg, True)
    return x


def fine_iteration(k, z, r, sz, idx, omg, backward):
    """level 0: the oracle's two colour calls, in place (ofst 0: colours 0, 1; ofst 1: colours 1, 0)"""
    cf = np.array([1, 1, 1, 1, 1, 1, 6], dtype=k.real)
    for color in (0, 1):
        k.psor2sma_core(z, sz, idx, cf, 1 if backward else 0, color, k.real(omg), r)


def apply(k, r, sz, idx, omg):
    """z = M^-1 r = V_0(r) on full S3D arrays; level 0 through the oracle's psor2sma_core (kernels k), the coarse levels numpy"""
    n0 = M.n0_of(idx)
    ins = M.inner(sz, idx)
    z = k.alloc(sz)
    if len(M.level_dims(n0)) == 1:
        for s in range(8):
            fine_iteration(k, z, r, sz, idx, omg, s >= 4)
        return z
    for _ in range(2):
        fine_iteration(k, z, r, sz, idx, omg, False)
    xc = vcycle(M.restrict(z[ins], r[ins], 0, n0), 1, n0, k.real(omg))
    z[ins] = M.prolong(z[ins], xc)
    for _ in range(2):
        fine_iteration(k, z, r, sz, idx, omg, True)
    return z


class CZ(M.CZ):
    """tests/mg_parity.CZ whose PCG also takes pc="mgrb" (the same exact-dot recipe)"""

    _mgrb = False

    def PCG(self, X, B, ItrMax, pc):
        self._mgrb = pc == "mgrb"
        return super().PCG(X, B, ItrMax, "mg" if self._mgrb else pc)

    def Preconditioner(self, xx, bb, pc):
        if not self._mgrb:
            return super().Preconditioner(xx, bb, pc)
        xx[...] = apply(self.k, bb, self.size, self.idx, self.ac1)
        self.cycles += 1


def run(gsz, itr_max, coef, prec="f32", dots="exact", perturb=0, with_error=False) -> O.Result:
    """``cz gsz pcg itr_max coef mgrb`` on the oracle"""
    cz = CZ(O.Kernels("oracle", prec), wide=dots is None, dots=dots, perturb=perturb)
    cz.setup(gsz, coef)
    itr, res = cz.PCG(cz.P, cz.RHS, itr_max, "mgrb")
    out = O.Result(itr=itr, res=res, history=cz.history, P=cz.P, dot_log=cz.dot_log)
    out.cycles = cz.cycles
    if with_error:
        out.errmax, out.errloc = cz.error_max()
    return out


def case(gsz, coef, prec, K, every_k=True):
    return dict(gsz=tuple(gsz), solver="pcg", pc="mgrb", coef=coef, prec=prec, K=K, every_k=every_k,
                id=f"pcg_mgrb_{'x'.join(map(str, gsz))}_{prec}_K{K}_w{coef}")


# K iterations each; FP32 premise and FP64 envelope checked on the CPU (tests/test_mgrb_oracle.py)
CASES = [
    case((9, 7, 12), 0.8, "f32", 3),
    case((9, 7, 12), 1.2, "f64", 3),
    case((33, 47, 61), 1.2, "f32", 4),
    case((33, 47, 61), 1.0, "f64", 4),
    case((64, 64, 64), 0.8, "f32", 4, every_k=False),
    case((64, 64, 64), 1.2, "f64", 4, every_k=False),
    case((40, 40, 1100), 0.8, "f64", 3, every_k=False),
]


def oracle(c, itr_max, perturb=0):
    return run(c["gsz"], itr_max, c["coef"], prec=c["prec"], dots="exact", perturb=perturb)


def premise_f32(c, r0=None):
    """mg_parity.premise_f32 on this file's oracle"""
    return M.premise_f32(c, r0 or oracle(c, c["K"]))


def envelope_f64(c, itr_max):
    """mg_parity.envelope_f64 on this file's oracle (it runs the module-level `oracle` of mg_parity: exchanged for the call)"""
    keep = M.oracle
    M.oracle = oracle
    try:
        return M.envelope_f64(c, itr_max)
    finally:
        M.oracle = keep
