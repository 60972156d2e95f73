"""A caller's own Poisson problem on the oracle (importable without a GPU): what tests/test_problem_oracle.py checks on the CPU and
tests/test_gpu_problem.py compares the GPU driver with.

The reference loops of oracle/cz_oracle.py call ``bc_k`` on the iterate after every checked iteration, which would overwrite a caller's
Dirichlet faces with those of the built-in test case.  `Kernels` below is oracle.cz_oracle.Kernels whose ``bc_k`` is the identity once
`user` is set (set-up still fills the built-in faces while it is not); tests/test_problem_oracle.py proves it harmless on the built-in
problem.  The solver class is tests/mgrb_parity.CZ (oracle.cz_oracle.CZ + PCG with none | jacobi | mg | mgrb), imported, not restated.

A problem is a right-hand side b and a field p on a box (ni, nj, nk), both indexed [i, j, k]: b random in [-1, 1] * 1e-2, p random in
[0, 1] (its outer layers are the Dirichlet values, the rest the initial guess), seeds fixed.  The padded arrays of the library and of the
oracle are [j + 2, i + 2, k + 2].
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mgrb_parity as RB  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

G = O.GUIDE
BOXES = [(9, 7, 12), (24, 20, 28), (33, 47, 61), (64, 64, 64)]
B_SCALE = 1e-2


class Kernels(O.Kernels):
    user = False

    def bc_k(self, sz, p, dh, org, nID):
        if not self.user:
            super().bc_k(sz, p, dh, org, nID)


def problem(gsz, prec, seed=0):
    """(b, p): the right-hand side and the field of a seeded random problem, C order [i, j, k]"""
    R = np.float32 if prec == "f32" else np.float64
    rng = np.random.default_rng(1000 + seed)
    b = ((rng.random(tuple(gsz)) * 2.0 - 1.0) * B_SCALE).astype(R)
    p = rng.random(tuple(gsz)).astype(R)
    return b, p


def pad(a, into=None):
    """the brick a[i, j, k] inside a padded array [j + 2, i + 2, k + 2] (zeros, or `into`, elsewhere)"""
    ni, nj, nk = a.shape
    out = np.zeros((nj + 2 * G, ni + 2 * G, nk + 2 * G), dtype=a.dtype) if into is None else into.copy()
    out[G:G + nj, G:G + ni, G:G + nk] = a.transpose(1, 0, 2)
    return out


def unpad(P):
    """the brick [i, j, k] of a padded array"""
    return np.ascontiguousarray(P[G:-G, G:-G, G:-G].transpose(1, 0, 2))


def case(gsz, solver, coef, prec, itr_max, pc=None, eps=None, seed=0):
    name = solver + ("_" + pc if pc else "")
    return dict(gsz=tuple(gsz), solver=solver, pc=pc, coef=coef, prec=prec, itr_max=itr_max, eps=eps, seed=seed,
                id=f"{name}_{'x'.join(map(str, gsz))}_{prec}")


def args(c, division=None):
    a = list(c["gsz"]) + [c["solver"], c["itr_max"], c["coef"]] + ([c["pc"]] if c["pc"] else [])
    return a + (list(division) if division else [])


def krylov(c):
    return c["solver"] in ("pbicgstab", "pcg")


def run(c, b=None, p=None, wrapped=True, perturb=0, itr_max=None, eps=None, builtin=False):
    """the oracle's solve of case c on the problem (b, p) (default: the seeded one; builtin: the test case set-up fills).  Stationary and
    line solvers with the wide residual sums the GPU is pinned to, the Krylov solvers with the exact dots of tests/*_parity.py."""
    k = Kernels("oracle", c["prec"])
    kr = krylov(c)
    cz = RB.CZ(k, wide=not kr, dots="exact" if kr else None, perturb=perturb)
    cz.setup(c["gsz"], c["coef"])
    k.user = wrapped
    if not builtin:
        if b is None:
            b, p = problem(c["gsz"], c["prec"], c["seed"])
        cz.P, cz.RHS = pad(p), pad(b)
    e = eps if eps is not None else c["eps"]
    if e is not None:
        cz.eps = e
    n = itr_max if itr_max is not None else c["itr_max"]
    s = c["solver"]
    if s in ("jacobi", "jacobi_maf"):
        itr, res = cz.JACOBI(cz.P, cz.RHS, n, maf=s.endswith("_maf"))
    elif s == "sor2sma":
        itr, res = cz.RBSOR(cz.P, cz.RHS, n)
    elif s == "psor":
        itr, res = cz.PSOR(cz.P, cz.RHS, n)
    elif s == "pcr_rb":
        itr, res = cz.LSOR_PCR_RB(cz.P, cz.RHS, n)
    elif s == "pcr":
        itr, res = cz.LSOR_PCR_VARIANT(cz.P, cz.RHS, n, s)
    elif s == "pbicgstab":
        itr, res = cz.PBiCGSTAB(cz.P, cz.RHS, n, c["pc"] or "none")
    elif s == "pcg":
        itr, res = cz.PCG(cz.P, cz.RHS, n, c["pc"] or "none")
    else:
        raise ValueError(s)
    return O.Result(itr=itr, res=res, history=cz.history, P=cz.P, dot_log=cz.dot_log)


def envelope_f64(c, **kw):
    """FP64 Krylov: the unperturbed run and the envelope of the runs with every dot at either edge of its summation bound (field, history)"""
    r = {q: run(c, perturb=q, **kw) for q in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr, (c["id"], [r[q].itr for q in (-1, 0, 1)])
    P0, h0 = r[0].P, np.array([v for _, v in r[0].history])
    E = np.maximum(np.abs(r[1].P - P0), np.abs(r[-1].P - P0))
    Eh = np.maximum(np.abs(np.array([v for _, v in r[1].history]) - h0), np.abs(np.array([v for _, v in r[-1].history]) - h0))
    return r[0], E, Eh


def f64_close(gpu, ref, env):
    """|gpu - ref| <= 2 env + 8 ulp(|ref|), elementwise (the bar of tests/test_gpu_pcg.py and tests/test_gpu_bicgstab_parity.py)"""
    gpu, ref, env = (np.asarray(v, dtype=np.float64) for v in (gpu, ref, env))
    bound = 2.0 * env + 8.0 * np.spacing(np.abs(ref))
    d = np.abs(gpu - ref)
    return bool(np.all(d <= bound)), float(np.max(d / np.maximum(bound, np.finfo(np.float64).tiny)))


def converged(c, r):
    """the solve stopped on its residual test within the iteration limit (BiCGSTAB's loop makes at most ItrMax - 1 iterations)"""
    last = c["itr_max"] - 1 if c["solver"] == "pbicgstab" else c["itr_max"]
    return 0 < r.itr <= last and len(r.history) == r.itr and r.res < (c["eps"] if c["eps"] is not None else O.EPS)


# Solver parity on a caller's problem: one case per family at least.  ItrMax and the boxes were chosen on the CPU so that every oracle run
# converges before ItrMax (tests/test_problem_oracle.py asserts it and, for the FP32 Krylov cases, the premise of bit equality: no dot of
# the run within its summation bound of a rounding boundary).
CASES = [
    case((24, 20, 28), "jacobi", 0.8, "f32", 4000),
    case((33, 47, 61), "jacobi", 0.9, "f64", 12000),
    case((33, 47, 61), "sor2sma", 1.5, "f32", 2000),
    case((64, 64, 64), "sor2sma", 1.7, "f64", 2000),
    case((24, 20, 28), "psor", 1.5, "f32", 1000),
    case((24, 20, 28), "pcr_rb", 1.2, "f32", 1000),
    case((33, 47, 61), "pcr", 1.2, "f64", 1000),
    case((24, 20, 28), "jacobi_maf", 0.8, "f32", 4000),
    case((33, 47, 61), "pbicgstab", 0.8, "f64", 200, pc="jacobi"),
    case((9, 7, 12), "pcg", 0.8, "f32", 100, pc="jacobi"),
    case((33, 47, 61), "pcg", 0.8, "f64", 300, pc="jacobi"),
    case((33, 47, 61), "pcg", 0.8, "f64", 100, pc="mg"),
    case((9, 7, 12), "pcg", 1.0, "f32", 100, pc="mgrb"),
    case((64, 64, 64), "pcg", 1.0, "f64", 100, pc="mgrb"),
]

# decomposed runs on the LOCAL transport (case, division): every rank imports its slice of one global array
DECOMP = [
    (case((40, 36, 44), "jacobi", 0.8, "f32", 4000), (2, 1, 2)),
    (case((41, 37, 45), "sor2sma", 1.5, "f32", 2000), (2, 2, 2)),
    (case((36, 40, 44), "jacobi", 0.9, "f64", 4000), (2, 2, 2)),
    (case((32, 36, 40), "pcg", 0.8, "f64", 100, pc="mg"), (2, 1, 2)),
    (case((32, 36, 40), "pcg", 0.8, "f32", 100, pc="jacobi"), (2, 2, 2)),
]

# solve with b1 (seed 0), set_rhs(b2) (seed RESOLVE_SEED), solve again from the first result.  The Jacobi case: the seed of b2 was chosen on
# the CPU so that the second solve converges at an iteration that is odd and no multiple of 3 -- not the last of a fused pass of two or of
# three sweeps, so the driver has to re-run the converged iteration alone (tests/test_problem_oracle.py asserts the count's residues).
RESOLVE_SEED = 5
RESOLVE = [case((33, 47, 61), "jacobi", 0.9, "f32", 12000), case((33, 47, 61), "sor2sma", 1.5, "f32", 2000),
           case((64, 64, 64), "pcg", 1.0, "f64", 100, pc="mgrb")]


def resolve(c):
    """the oracle's two solves of a RESOLVE case: (first, second)"""
    b1, p = problem(c["gsz"], c["prec"], 0)
    b2, _ = problem(c["gsz"], c["prec"], RESOLVE_SEED)
    first = run(c, b=b1, p=p)
    return first, run(c, b=b2, p=unpad(first.P))


def manufactured(gsz):
    """(u, b, p) in FP64: a smooth u, b = A u made by the oracle's blas_calc_ax, p = u on the faces and zero inside"""
    k = Kernels("oracle", "f64")
    x, y, z = (np.linspace(0.0, 1.0, n) for n in gsz)
    u = (np.sin(2.0 * x)[:, None, None] * np.cos(1.5 * y)[None, :, None] * np.exp(0.5 * z)[None, None, :] + x[:, None, None] * z[None, None, :])
    U = pad(np.ascontiguousarray(u))
    idx, _ = O.range_inner_index(list(gsz), [-1] * 6)
    AU = k.alloc(list(gsz))
    k.blas_calc_ax(AU, U, list(gsz), idx, np.array([1, 1, 1, 1, 1, 1, 6], dtype=np.float64))
    p = np.ascontiguousarray(u).copy()
    p[1:-1, 1:-1, 1:-1] = 0.0
    return np.ascontiguousarray(u), unpad(AU), p
