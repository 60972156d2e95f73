"""The red-black V-cycle of `pcg ... mgrb` on the CPU (tests/mgrb_parity.py): its level-0 iterations are the oracle's colour calls, it is a
symmetric definite preconditioner for every coefficient offered, PCG with it converges in the iteration counts DESIGN.md §5.10.2 states
(fewer than `mg`'s), and the GPU cases of tests/test_gpu_mgrb.py satisfy the premises of their bars."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_parity as M  # noqa: E402
import mgrb_parity as RB  # noqa: E402
import test_mg_oracle as TM  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

OMEGAS = (0.8, 1.0, 1.2)  # the coefficients tested; (0, RB.OMG_MAX] is what the command line accepts
MG_COUNTS = {64: 8, 128: 9}  # `mg` at coefficient 0.8


def _apply(k, sz, idx, v_inner, omg=0.8):
    r = k.alloc(sz)
    ins = M.inner(sz, idx)
    r[ins] = v_inner
    return RB.apply(k, r, sz, idx, omg)[ins]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_level0_iterations_are_the_oracles_colour_calls(prec):
    """colour c of the restatement is the oracle's psor2sma_core with ofst + color = c (mod 2) on a single domain, so F is its colour calls
    0, 1 with ofst 0 and B the same calls with ofst 1 -- and B is also the calls 1, 0 with ofst 0"""
    k = O.Kernels("oracle", prec)
    R = k.real
    cf = np.array([1, 1, 1, 1, 1, 1, 6], dtype=R)
    sz, idx, n0 = TM._box((33, 47, 61))
    ins = M.inner(sz, idx)
    rng = np.random.default_rng(3)
    u, b = k.alloc(sz), k.alloc(sz)
    u[ins], b[ins] = rng.standard_normal(u[ins].shape).astype(R), rng.standard_normal(b[ins].shape).astype(R)
    for c in (0, 1):
        for ofst in (0, 1):
            ref = u.copy()
            k.psor2sma_core(ref, sz, idx, cf, ofst, (c + ofst) & 1, R(1.2), b)
            assert RB.sweep(u[ins], b[ins], 0, n0, 1.2, c).tobytes() == ref[ins].tobytes(), (c, ofst)
    for backward in (False, True):
        want = RB.iteration(u[ins], b[ins], 0, n0, 1.2, backward)
        got = u.copy()
        RB.fine_iteration(k, got, b, sz, idx, 1.2, backward)
        assert got[ins].tobytes() == want.tobytes(), backward
        other = u.copy()  # the two colour calls in the other order, ofst 0
        for color in ((1, 0) if backward else (0, 1)):
            k.psor2sma_core(other, sz, idx, cf, 0, color, R(1.2), b)
        assert other.tobytes() == got.tobytes(), backward
    # from zero: u = None is u = 0
    z = np.zeros_like(b[ins])
    assert RB.iteration(None, b[ins], 0, n0, 0.8, False).tobytes() == RB.iteration(z, b[ins], 0, n0, 0.8, False).tobytes()


@pytest.mark.parametrize("gsz", [(9, 7, 12), (33, 47, 61), (6, 6, 6)])
def test_apply_level0_through_the_oracle_equals_numpy(gsz):
    """the whole cycle with level 0 through psor2sma_core is the numpy cycle at every level"""
    for prec in ("f32", "f64"):
        k = O.Kernels("oracle", prec)
        sz, idx, n0 = TM._box(gsz)
        v = np.random.default_rng(4).standard_normal((n0[1], n0[0], n0[2])).astype(k.real)
        assert _apply(k, sz, idx, v, 1.2).tobytes() == RB.vcycle(v, 0, n0, k.real(1.2)).tobytes()


@pytest.mark.parametrize("omg", OMEGAS)
def test_preconditioner_is_symmetric(omg, monkeypatch):
    """test_mg_oracle's construction and tolerance ((M r1).r2 = r1.(M r2) to 1e-12 relative, FP64) on this cycle"""
    monkeypatch.setattr(TM, "_apply", functools.partial(_apply, omg=omg))
    TM.test_preconditioner_is_symmetric()


@pytest.mark.parametrize("omg", OMEGAS)
@pytest.mark.parametrize("gsz", [(34, 34, 34), (33, 47, 61), (40, 40, 1100)])
def test_preconditioned_operator_is_definite(gsz, omg, monkeypatch):
    """the smallest Ritz value of M A (test_mg_oracle's Lanczos) stays positive for every coefficient offered; printed for DESIGN.md"""
    monkeypatch.setattr(TM, "_apply", _apply)
    lo = TM._smallest_ritz(gsz, omg)
    print(f"smallest Ritz value of M A, {gsz}, omega {omg}: {lo:.4f}")
    assert lo > 0.0, (gsz, omg, lo)
    assert omg <= RB.OMG_MAX


def test_oracle_iteration_counts():
    """PCG with the red-black cycle, FP64, exact dots, eps 1e-5.  The gate of the feature: at coefficient 0.8 strictly fewer iterations than
    `mg`'s 9 at 128^3 and no more than its 8 at 64^3.  The counts at the larger coefficients are those DESIGN.md §5.10.2 records."""
    counts = {}
    for n in (64, 128):
        for omg in OMEGAS:
            r = RB.run((n, n, n), 1000, omg, prec="f64")
            assert r.res < O.EPS and r.cycles == r.itr
            counts[n, omg] = r.itr
    print("mgrb iteration counts", counts)
    assert M.run((64, 64, 64), 1000, 0.8, prec="f64").itr == MG_COUNTS[64]
    assert counts[128, 0.8] < MG_COUNTS[128] and counts[64, 0.8] <= MG_COUNTS[64], counts
    assert counts == {(64, 0.8): 7, (64, 1.0): 5, (64, 1.2): 5, (128, 0.8): 8, (128, 1.0): 6, (128, 1.2): 5}, counts


@pytest.mark.parametrize("c", RB.CASES, ids=[c["id"] for c in RB.CASES])
def test_pcg_mgrb_parity_premise(c):
    """the GPU cases of tests/test_gpu_mgrb.py: FP32 no dot within its summation bound of a rounding boundary; FP64 an envelope that says
    something"""
    if c["prec"] == "f32":
        r0 = RB.premise_f32(c)
        for p in (-1, 1):
            rp = RB.oracle(c, c["K"], p)
            assert rp.itr == r0.itr and rp.history == r0.history and rp.P.tobytes() == r0.P.tobytes(), (c["id"], p)
    else:
        RB.envelope_f64(c, c["K"])
