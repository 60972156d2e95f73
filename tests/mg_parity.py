"""The multigrid V-cycle preconditioner of `pcg ... mg` restated in numpy (importable without a GPU), and PCG with it on the oracle.

DESIGN.md §5.10 fixes the cycle down to the bit; this is that text as code:

* levels: level 0 is the inner box, level l+1 has ceil(n/2) points per direction, coarsening stops at the first level whose largest extent
  is <= 4 (the coarsest);
* level l's operator has the face weights Wx = Ey Ez, Wy = Ex Ez, Wz = Ex Ey (E the extent of a coarse point in level-0 points) and
  D = 2 (Wx + Wy + Wz), and the correction is zero outside the box;
* smooth: pn = pp + ((ss - bb)/D - pp) omg, ss summed in the reference's c1 .. c6 order, every operation rounded to REAL;
* restrict: the residual b - (ss - D x) summed over the <= 8 children, pairs along k, then i, then j (absent children drop out);
* prolong: u = x + R(R(1.8) x_c(parent));
* V_l(b): 2 sweeps from zero, restrict, x_c = V_{l+1}, prolong, 2 sweeps (the coarsest: 8 sweeps from zero).  Level 0's sweeps are the
  oracle's C jacobi (oracle.cz_oracle.Kernels), the coarse levels this file's numpy.

Arrays here are the inner boxes of the levels, shape (nj, ni, nk) (K fastest, as the S3D layout); `pad` puts the zero faces around one.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cg_parity as CP  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

ALPHA = 1.8
COARSEST = 4


def level_dims(n0):
    """points per direction (ni, nj, nk) of every level, level 0 = n0"""
    dims = [tuple(int(v) for v in n0)]
    while max(dims[-1]) > COARSEST:
        dims.append(tuple((v + 1) // 2 for v in dims[-1]))
    return dims


def extents(n0d, level, n):
    """E(I) = min(2^l, n0 - I 2^l), I = 0 .. n-1"""
    s = 1 << level
    return np.minimum(s, n0d - np.arange(n) * s)


def weights(n0, level, R):
    """Wx, Wy, Wz, D of every point of the level, shape (nj, ni, nk), in REAL (small integers: exact)"""
    ni, nj, nk = level_dims(n0)[level]
    ex, ey, ez = extents(n0[0], level, ni), extents(n0[1], level, nj), extents(n0[2], level, nk)
    shape = (nj, ni, nk)
    wx = np.broadcast_to(ey[:, None, None] * ez[None, None, :], shape)
    wy = np.broadcast_to(ex[None, :, None] * ez[None, None, :], shape)
    wz = np.broadcast_to(ey[:, None, None] * ex[None, :, None], shape)
    return wx.astype(R), wy.astype(R), wz.astype(R), (2 * (wx + wy + wz)).astype(R)


def pad(a):
    return np.pad(a, 1)


def _ss(u, W):
    wx, wy, wz, _ = W
    p = pad(u)
    ip, im = p[1:-1, 2:, 1:-1], p[1:-1, :-2, 1:-1]
    jp, jm = p[2:, 1:-1, 1:-1], p[:-2, 1:-1, 1:-1]
    kp, km = p[1:-1, 1:-1, 2:], p[1:-1, 1:-1, :-2]
    return wx * ip + wx * im + wy * jp + wy * jm + wz * kp + wz * km  # left to right: the c1 .. c6 order


def smooth(u, b, level, n0, omg):
    """one relaxed Jacobi sweep of the level (u None: from zero)"""
    R = b.dtype.type
    W = weights(n0, level, R)
    if u is None:
        u = np.zeros_like(b)
    ss = _ss(u, W)
    dp = ((ss - b) / W[3] - u) * R(omg)
    return u + dp


def residual(x, b, level, n0):
    W = weights(n0, level, b.dtype.type)
    return b - (_ss(x, W) - W[3] * x)


def _pair(a, axis):
    """children 2I and 2I+1 along axis summed; a lone last child stays alone"""
    a = np.moveaxis(a, axis, 0)
    lo, hi = a[0::2], a[1::2]
    out = lo.copy()
    out[: hi.shape[0]] = lo[: hi.shape[0]] + hi
    return np.moveaxis(out, 0, axis)


def restrict(x, b, level, n0):
    """b_{l+1} = the residual summed over the children: ((r000 + r001) + (r010 + r011)) + ((r100 + r101) + (r110 + r111)), (j, i, k)"""
    r = residual(x, b, level, n0)
    return _pair(_pair(_pair(r, 2), 1), 0)


def prolong(x, xc):
    R = x.dtype.type
    nj, ni, nk = x.shape
    up = np.repeat(np.repeat(np.repeat(xc, 2, 0), 2, 1), 2, 2)[:nj, :ni, :nk]
    c = R(ALPHA) * up
    return x + c


def vcycle(b, level, n0, omg):
    """x = V_l(b) on the coarse levels (numpy at every level, level 0 included)"""
    nlev = len(level_dims(n0))
    if level == nlev - 1:
        x = smooth(None, b, level, n0, omg)
        for _ in range(7):
            x = smooth(x, b, level, n0, omg)
        return x
    x = smooth(smooth(None, b, level, n0, omg), b, level, n0, omg)
    xc = vcycle(restrict(x, b, level, n0), level + 1, n0, omg)
    u = prolong(x, xc)
    return smooth(smooth(u, b, level, n0, omg), b, level, n0, omg)


def inner(sz, idx, g=O.GUIDE):
    ist, ied, jst, jed, kst, ked = idx
    return (slice(jst + g - 1, jed + g), slice(ist + g - 1, ied + g), slice(kst + g - 1, ked + g))


def n0_of(idx):
    return (idx[1] - idx[0] + 1, idx[3] - idx[2] + 1, idx[5] - idx[4] + 1)


def apply(k, r, sz, idx, omg):
    """z = M^-1 r = V_0(r) on full S3D arrays; level 0's sweeps through the oracle's jacobi (kernels k), the coarse levels numpy"""
    R = k.real
    cf = np.array([1, 1, 1, 1, 1, 1, 6], dtype=R)
    omg = R(omg)
    n0 = n0_of(idx)
    ins = inner(sz, idx)
    z, wk2 = k.alloc(sz), k.alloc(sz)

    def sweeps(n):
        for _ in range(n):
            k.jacobi(z, sz, idx, cf, omg, r, wk2)

    if len(level_dims(n0)) == 1:
        sweeps(O.LC_MAX)
        return z
    sweeps(2)
    xc = vcycle(restrict(z[ins], r[ins], 0, n0), 1, n0, omg)
    z[ins] = prolong(z[ins], xc)
    sweeps(2)
    return z


class CZ(CP.CZ):
    """tests/cg_parity.CZ whose PCG also takes pc="mg" (M^-1 = the V-cycle above; the same exact-dot recipe)"""

    _mg = False

    def PCG(self, X, B, ItrMax, pc):
        self._mg = pc == "mg"
        self.cycles = 0
        return super().PCG(X, B, ItrMax, "jacobi" if self._mg else pc)

    def Preconditioner(self, xx, bb, pc):
        if not self._mg:
            return super().Preconditioner(xx, bb, pc)
        xx[...] = apply(self.k, bb, self.size, self.idx, self.ac1)
        self.cycles += 1


def run(gsz, itr_max, coef, prec="f32", dots="exact", perturb=0, with_error=False) -> O.Result:
    """``cz gsz pcg itr_max coef mg`` on the oracle"""
    cz = CZ(O.Kernels("oracle", prec), wide=dots is None, dots=dots, perturb=perturb)
    cz.setup(gsz, coef)
    itr, res = cz.PCG(cz.P, cz.RHS, itr_max, "mg")
    out = O.Result(itr=itr, res=res, history=cz.history, P=cz.P, dot_log=cz.dot_log)
    out.cycles = cz.cycles
    if with_error:
        out.errmax, out.errloc = cz.error_max()
    return out


def case(gsz, coef, prec, K, every_k=True):
    return dict(gsz=tuple(gsz), solver="pcg", pc="mg", coef=coef, prec=prec, K=K, every_k=every_k,
                id=f"pcg_mg_{'x'.join(map(str, gsz))}_{prec}_K{K}")


# K iterations each; FP32 premise and FP64 envelope checked on the CPU (tests/test_mg_oracle.py)
CASES = [
    case((9, 7, 12), 0.8, "f32", 3),
    case((9, 7, 12), 0.8, "f64", 3),
    case((33, 47, 61), 0.8, "f32", 4),
    case((33, 47, 61), 1.0, "f64", 4),
    case((64, 64, 64), 0.8, "f32", 4, every_k=False),
    case((64, 64, 64), 0.8, "f64", 4, every_k=False),
    case((40, 40, 1100), 0.8, "f64", 3, every_k=False),
]


def oracle(c, itr_max, perturb=0):
    return run(c["gsz"], itr_max, c["coef"], prec=c["prec"], dots="exact", perturb=perturb)


def premise_f32(c, r0=None):
    """FP32: no summation order can flip a rounding through iteration K (the unperturbed K-iteration run)"""
    r0 = r0 or oracle(c, c["K"])
    f = CP.flips(r0, "f32")
    assert not f, f"{c['id']}: premise fails (choose another case): dots within their summation bound of a float boundary {f[:4]}"
    return r0


def envelope_f64(c, itr_max):
    """FP64: the unperturbed run and the envelope of the two perturbed ones, field and history"""
    r = {p: oracle(c, itr_max, p) for p in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr, (c["id"], itr_max, [r[p].itr for p in (-1, 0, 1)])
    P0, h0 = r[0].P, np.array([v for _, v in r[0].history])
    E = np.maximum(np.abs(r[1].P - P0), np.abs(r[-1].P - P0))
    Eh = np.maximum(np.abs(np.array([v for _, v in r[1].history]) - h0), np.abs(np.array([v for _, v in r[-1].history]) - h0))
    rel = max(float(E.max() / np.abs(P0).max()), float((Eh / h0).max()) if len(h0) else 0.0)
    assert rel <= CP.ENVELOPE_MAX, f"{c['id']}: FP64 envelope {rel:.2e} relative at ItrMax {itr_max}"
    return r[0], E, Eh
