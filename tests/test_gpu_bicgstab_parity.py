"""BiCGSTAB iteration by iteration against the exact-dot oracle (-m gpu).

The other BiCGSTAB tests bound a whole solve by tolerances fitted to the reference's REAL-accumulated dot products (1e-3 in FP32).  Here the
GPU driver (cubez_amd.CZ) runs K iterations and is compared after every iteration with the oracle whose dot products are correctly rounded
(oracle/cz_oracle.py, dots="exact"; tests/bicg_parity.py explains the bound).  Every other kernel of the oracle is the C restatement the
stationary tests pin bit for bit, so what is tested here is the driver's composition: the scalar recurrence, which vector each fused dot
reads, when alpha / omega are read (on the device or on the host), the vector updates made inside the preconditioner's first pass, the p_ / s_
aliasing of a copying preconditioner, and the all-reduce of a decomposed run.

* FP32: field, history and iteration count bit for bit (`tobytes()` / `==`): no tolerance anywhere.
* FP64: |GPU - P0| <= 2 E + 8 ulp(|P0|) elementwise, E the envelope of the oracle runs with every dot at either edge of its summation bound.
  E is derived, not fitted; the factor 2 and the 8 ulp are margins on it (the GPU's dots lie inside the bound, not at an edge, and the last
  vector updates round once more), not numbers tuned to make a run pass.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bicg_parity as BP  # noqa: E402

pytestmark = pytest.mark.gpu


def _gpu(c, itr_max):
    from cubez_amd import CZ
    cz = CZ(c["prec"], quiet=True)
    try:
        assert cz.setup(BP.args(c, itr_max)) == 1
        itr = cz.solve()
        return dict(itr=itr, hist=list(cz.history()), P=cz.field(), info=cz.info())
    finally:
        cz.close()


def _f64_close(gpu, ref, env):
    """|gpu - ref| <= 2 env + 8 ulp(|ref|), elementwise; returns the worst ratio for the message"""
    gpu, ref, env = (np.asarray(v, dtype=np.float64) for v in (gpu, ref, env))
    bound = 2.0 * env + 8.0 * np.spacing(np.abs(ref))
    d = np.abs(gpu - ref)
    return bool(np.all(d <= bound)), float(np.max(d / np.maximum(bound, np.finfo(np.float64).tiny)))


def _check(c, run=_gpu):
    """the GPU after each compared iteration count k (ItrMax = k + 1) and the K-iteration history, against the exact-dot oracle"""
    K = c["K"]
    for k in BP.ks(c):
        g = run(c, k + 1)
        if c["prec"] == "f32":
            o = BP.oracle(c, k + 1)
            if k == K:
                BP.premise_f32(c, o, perturbed=False)  # (the full premise, +-1 runs included, is tests/test_oracle.py's)
            assert g["itr"] == o.itr, (c["id"], k, g["itr"], o.itr)
            assert g["P"].tobytes() == o.P.tobytes(), f"{c['id']}: field differs from the exact-dot oracle after {k} iterations"
            if k == K:
                assert g["hist"] == [r for _, r in o.history], (c["id"], g["hist"], o.history)
        else:
            o, E, Eh = BP.envelope_f64(c, k + 1)
            assert g["itr"] == o.itr, (c["id"], k, g["itr"], o.itr)
            ok, worst = _f64_close(g["P"], o.P, E)
            assert ok, f"{c['id']}: field beyond the derived bound after {k} iterations (worst |d| / bound = {worst:.3g})"
            if k == K:
                h0 = [r for _, r in o.history]
                assert len(g["hist"]) == len(h0)
                ok, worst = _f64_close(g["hist"], h0, Eh)
                assert ok, f"{c['id']}: history beyond the derived bound (worst |d| / bound = {worst:.3g})"
    return g


@pytest.mark.parametrize("c", BP.CASES, ids=[c["id"] for c in BP.CASES])
def test_bicgstab_iterations_vs_exact_dot_oracle(c):
    g = _check(c)
    if c["gsz"] == (64, 64, 64) and c["pc"] == "jacobi":
        assert g["info"]["bicg_fused"] > 0, g["info"]  # the preconditioner's whole-box fused pass made the vector updates


@pytest.mark.parametrize("switch", ["CZ_BICG_FUSE", "CZ_BICG_DEVSC", "CZ_BICG_ALIAS"])
@pytest.mark.parametrize("c", BP.SWITCH_CASES, ids=[c["id"] for c in BP.SWITCH_CASES])
def test_bicgstab_switch_off_vs_exact_dot_oracle(c, switch, monkeypatch):
    """each switch of the iteration turned off, against the oracle (the default form is test_bicgstab_iterations_vs_exact_dot_oracle)"""
    monkeypatch.setenv(switch, "0")
    g = _check(c)
    if switch == "CZ_BICG_FUSE":
        assert g["info"]["bicg_fused"] == 0, g["info"]


@pytest.mark.parametrize("c", BP.DECOMP_CASES, ids=[c["id"] for c in BP.DECOMP_CASES])
def test_decomposed_bicgstab_vs_exact_dot_oracle(c):
    """ranks as threads on the LOCAL transport, division (2, 1, 2): the all-reduce of double partials is one more summation order, so the same
    bounds hold -- FP32 bit for bit."""
    from test_gpu_decomp import _decomposed

    def run(c, itr_max):
        results, G = _decomposed(c["prec"], c["gsz"], c["solver"], itr_max, c["coef"], (2, 1, 2), c["pc"])
        assert all(r[0] == results[0][0] and r[2] == results[0][2] for r in results)
        return dict(itr=results[0][0], hist=list(results[0][2]), P=G, info=results[0][4]["info"])

    # the assembled field holds the owned cells only: compare on the inner box with the oracle's faces written in
    def run_full(c, itr_max):
        g = run(c, itr_max)
        o = BP.oracle(c, 2)  # any run: the faces (boundary values) are set once and never written
        P = o.P.copy()
        P[2:-2, 2:-2, 2:-2] = g["P"][2:-2, 2:-2, 2:-2]
        g["P"] = P
        return g

    _check(c, run_full)
