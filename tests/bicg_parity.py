"""Cases and oracle-side premise of tests/test_gpu_bicgstab_parity.py (importable without a GPU; tests/test_oracle.py runs the premise).

The GPU sums every dot product of BiCGSTAB over per-point products taken in REAL, in double, in some fixed order; the oracle's exact-dot
mode (oracle/cz_oracle.py, dots="exact") sums the same products correctly rounded to S and knows the bound B = gamma_(n-1) sum |t_i| on how
far ANY order of double summation lies from S.  So the GPU's dot lies in [S - B, S + B] and, rounded to REAL, in [R(S - B), R(S + B)].

* FP32: where every dot of the oracle run has R(S - B) == R(S + B), no summation order can move a single bit -- the GPU must equal the oracle
  bit for bit (field, history, count).  premise_f32() checks exactly that, on the log of the unperturbed run, and that the runs with every
  dot pushed to either edge (perturb = -1 / +1) are bit-identical to it.
* FP64: the runs with every dot at -B / +B bound how far the trajectory can move: the envelope E = max(|P+ - P0|, |P- - P0|).
  envelope_f64() computes it and checks that it stays small (<= 1e-8 relative), so that the GPU bound built from it has teeth.
"""
from __future__ import annotations

import numpy as np

from oracle import cz_oracle as O

ENVELOPE_MAX = 1e-8  # FP64: the envelope must stay below this (relative), or the case is too long to say anything


def case(gsz, solver, pc, coef, prec, K, every_k=True):
    return dict(gsz=tuple(gsz), solver=solver, pc=pc, coef=coef, prec=prec, K=K, every_k=every_k,
                id=f"{solver}_{pc}_{'x'.join(map(str, gsz))}_{prec}_K{K}")


# K iterations each: the BiCGSTAB loop is `for (itr = 1; itr < ItrMax; itr++)` (cz_driver.cpp, cz_Poisson.cpp:373), so ItrMax = K + 1.
# Chosen on the CPU with premise_f32 / envelope_f64 below (tests/test_oracle.py::test_bicgstab_parity_premise).
CASES = [
    # every preconditioner name of the reference, FP32 and FP64, over the shape groups
    case((33, 47, 61), "pbicgstab", "none", 0.8, "f32", 5),
    case((9, 7, 12), "pbicgstab", "none", 0.8, "f64", 3),
    case((64, 64, 64), "pbicgstab", "jacobi", 0.8, "f32", 4),       # whole-box fused preconditioner pass (bicg_fused > 0)
    case((64, 64, 64), "pbicgstab", "jacobi", 0.8, "f64", 4),
    case((40, 36, 61), "pbicgstab", "sor2sma", 1.5, "f32", 5),
    case((33, 47, 61), "pbicgstab", "sor2sma", 1.5, "f64", 4),
    case((33, 47, 61), "pbicgstab", "psor", 1.2, "f32", 4),
    case((40, 36, 61), "pbicgstab", "psor", 1.2, "f64", 4),
    case((40, 36, 61), "pbicgstab", "pcr", 1.2, "f32", 4),
    case((33, 47, 61), "pbicgstab", "pcr", 1.2, "f64", 4),
    case((33, 47, 61), "pbicgstab", "pcr_rb", 1.2, "f32", 4),
    case((40, 36, 61), "pbicgstab", "pcr_rb", 1.2, "f64", 4),
    # (no pcr_esa: like the reference's (cz_Evaluate.cpp:570-620), the command line takes pcr_esa as a solver only, not as a preconditioner)
    case((9, 7, 12), "pbicgstab", "jacobi", 0.8, "f32", 3),
    case((40, 36, 61), "pbicgstab", "pcr_eda", 1.2, "f32", 4),
    case((33, 47, 61), "pbicgstab", "pcr_eda", 1.2, "f64", 4),
    case((33, 47, 61), "pbicgstab", "pcr_rb_esa", 1.2, "f32", 4),
    case((40, 36, 61), "pbicgstab", "pcr_rb_esa", 1.2, "f64", 4),
    case((40, 36, 61), "pbicgstab", "pcr_j_esa", 0.9, "f32", 4),
    case((33, 47, 61), "pbicgstab", "pcr_j_esa", 0.9, "f64", 4),
    # the MAF flavour
    case((33, 47, 61), "pbicgstab_maf", "jacobi_maf", 0.8, "f32", 4),
    case((40, 36, 61), "pbicgstab_maf", "sor2sma_maf", 1.5, "f64", 4),
    case((33, 47, 61), "pbicgstab_maf", "pcr_rb_maf", 1.2, "f64", 4),
    case((40, 36, 61), "pbicgstab_maf", "jacobi", 0.8, "f32", 4),
    # k extent > 1 028: the k-windowed pass (FP64 rows beyond 1 020 elements)
    case((40, 40, 1100), "pbicgstab", "jacobi", 0.3, "f64", 3),
    case((40, 40, 1100), "pbicgstab", "jacobi", 0.3, "f32", 3),
    # configs[3]'s preconditioner at 128^3 (n ~ 2e6: the premise is not trivial there; coefficient 0.9 -- with 0.8 a dot of iteration 3 lies
    # within its summation bound of a float rounding boundary, so no summation-order-free statement can be made beyond iteration 2)
    case((128, 128, 128), "pbicgstab", "jacobi", 0.9, "f32", 5, every_k=False),
]

# the iteration's switches against the oracle (not only against each other)
SWITCH_CASES = [c for c in CASES if (c["pc"], c["gsz"]) in ((("jacobi", (64, 64, 64))), ("sor2sma", (40, 36, 61))) and c["solver"] == "pbicgstab"]
SWITCH_CASES.append(CASES[1])  # FP64 none
# decomposed runs (LOCAL transport, division (2, 1, 2))
DECOMP_CASES = [case((32, 36, 40), "pbicgstab", pc, cf, prec, 4, every_k=False)
                for pc, cf in (("jacobi", 0.8), ("sor2sma", 1.5)) for prec in ("f32", "f64")]


def ks(c):
    """the iteration counts whose fields are compared"""
    return list(range(1, c["K"] + 1)) if c["every_k"] else [1, c["K"]]


def args(c, itr_max):
    return list(c["gsz"]) + [c["solver"], itr_max, c["coef"], c["pc"]]


def oracle(c, itr_max, perturb=0):
    return O.run(c["gsz"], c["solver"], itr_max, c["coef"], c["pc"], kind="oracle", prec=c["prec"], dots="exact", perturb=perturb)


def flips(r, prec):
    """dots of an exact-dot run whose two edges round to different REALs: (itr, which) of each"""
    R = np.float32 if prec == "f32" else np.float64
    return [(i, w) for (i, w, S, B, _) in r.dot_log if R(S - B) != R(S + B)]


def premise_f32(c, r0=None, perturbed=True):
    """FP32: no summation order can flip a rounding through iteration K.  Returns the unperturbed K-iteration run."""
    r0 = r0 or oracle(c, c["K"] + 1)
    f = flips(r0, "f32")
    assert not f, f"{c['id']}: premise fails (choose another case): dots within their summation bound of a float boundary {f[:4]}"
    if perturbed:
        for p in (-1, 1):
            rp = oracle(c, c["K"] + 1, p)
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
