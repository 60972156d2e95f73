"""PCG on the GPU (-m gpu) iteration by iteration against the exact-dot oracle of tests/cg_parity.py, its two fused kernels alone, and the
command line's refusals.

Bars as in tests/test_gpu_bicgstab_parity.py (where they are explained):
* FP32: field, history and iteration count bit for bit.
* FP64: |GPU - P0| <= 2 E + 8 ulp(|P0|) elementwise, E the envelope of the oracle runs with every dot at either edge of its summation bound.
"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cg_parity as CP  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu(c, itr_max):
    from cubez_amd import CZ
    cz = CZ(c["prec"], quiet=True)
    try:
        assert cz.setup(CP.args(c, itr_max)) == 1
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
    """the GPU after each compared iteration count k (ItrMax = k) and the K-iteration history, against the exact-dot oracle"""
    K = c["K"]
    for k in CP.ks(c):
        g = run(c, k)
        if c["prec"] == "f32":
            o = CP.oracle(c, k)
            if k == K:
                CP.premise_f32(c, o, perturbed=False)  # (the full premise is tests/test_cg_oracle.py's)
            assert g["itr"] == o.itr, (c["id"], k, g["itr"], o.itr)
            assert g["P"].tobytes() == o.P.tobytes(), f"{c['id']}: field differs from the exact-dot oracle after {k} iterations"
            if k == K:
                assert g["hist"] == [r for _, r in o.history], (c["id"], g["hist"], o.history)
        else:
            o, E, Eh = CP.envelope_f64(c, k)
            assert g["itr"] == o.itr, (c["id"], k, g["itr"], o.itr)
            ok, worst = _f64_close(g["P"], o.P, E)
            assert ok, f"{c['id']}: field beyond the derived bound after {k} iterations (worst |d| / bound = {worst:.3g})"
            if k == K:
                h0 = [r for _, r in o.history]
                assert len(g["hist"]) == len(h0)
                ok, worst = _f64_close(g["hist"], h0, Eh)
                assert ok, f"{c['id']}: history beyond the derived bound (worst |d| / bound = {worst:.3g})"
    return g


@pytest.mark.parametrize("c", CP.CASES, ids=[c["id"] for c in CP.CASES])
def test_pcg_iterations_vs_exact_dot_oracle(c):
    g = _check(c)
    assert g["info"]["cg_fused"] == c["K"], g["info"]  # single domain: every direction was made inside the SpMV pass


@pytest.mark.parametrize("c", CP.SWITCH_CASES, ids=[c["id"] for c in CP.SWITCH_CASES])
def test_pcg_unfused_vs_exact_dot_oracle(c, monkeypatch):
    """CZ_CG_FUSE=0: the separate update, SpMV and dot launches, against the same oracle"""
    monkeypatch.setenv("CZ_CG_FUSE", "0")
    g = _check(c)
    assert g["info"]["cg_fused"] == 0, g["info"]


@pytest.mark.parametrize("c", CP.DECOMP_CASES, ids=[c["id"] for c in CP.DECOMP_CASES])
def test_decomposed_pcg_vs_exact_dot_oracle(c):
    """ranks as threads on the LOCAL transport, division (2, 1, 2): the direction takes the unfused path (cg_fused == 0), the all-reduce of
    double partials is one more summation order, so the same bounds hold"""
    from test_gpu_decomp import _decomposed

    def run(c, itr_max):
        results, G = _decomposed(c["prec"], c["gsz"], "pcg", itr_max, c["coef"], (2, 1, 2), c["pc"])
        assert all(r[0] == results[0][0] and r[2] == results[0][2] for r in results)
        assert all(r[4]["info"]["cg_fused"] == 0 for r in results)
        o = CP.oracle(c, 1)  # the faces (boundary values) are set once and never written
        P = o.P.copy()
        P[2:-2, 2:-2, 2:-2] = G[2:-2, 2:-2, 2:-2]
        return dict(itr=results[0][0], hist=list(results[0][2]), P=P, info=results[0][4]["info"])

    _check(c, run)


def test_pcg_two_rccl_ranks_equal_single_domain():
    """two processes over RCCL (tests/rccl_rank_worker.py), division (2, 1, 1), FP32: bit-equal to the single-domain run"""
    from test_gpu_rccl import run_ranks, single
    c = CP.DECOMP_CASES[2]  # jacobi, f32 (premise: tests/test_cg_oracle.py)
    assert c["pc"] == "jacobi" and c["prec"] == "f32"
    itr1, res1, hist1, P1 = single("f32", c["gsz"], "pcg", c["K"], c["coef"], "jacobi")
    recs, G, logs = run_ranks("f32", c["gsz"], "pcg", c["K"], c["coef"], (2, 1, 1), pc="jacobi")
    assert G[2:-2, 2:-2, 2:-2].tobytes() == P1[2:-2, 2:-2, 2:-2].tobytes()
    for rec in recs:
        assert rec["info"]["rccl_ranks"] == 2 and rec["info"]["cg_fused"] == 0, rec["info"]
        assert rec["itr"] == itr1 == c["K"] and rec["history"] == list(hist1)


@pytest.mark.parametrize("pc", ["none", "jacobi"])
def test_pcg_64cube_f64_to_convergence(pc):
    """the whole solve: the count equals the oracle's (every perturbed oracle run agrees on it), the analytic error within 2 E + 8 ulp, E the
    envelope of the perturbed runs' error"""
    from cubez_amd import CZ
    r = {p: CP.run((64, 64, 64), 1000, 0.8, pc, prec="f64", perturb=p, with_error=True) for p in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr < 1000
    cz = CZ("f64", quiet=True)
    try:
        assert cz.setup([64, 64, 64, "pcg", 1000, 0.8, pc]) == 1
        itr = cz.solve()
        err = cz.error_max()[0]
        info = cz.info()
    finally:
        cz.close()
    assert itr == r[0].itr, (itr, r[0].itr)
    assert info["cg_fused"] == itr
    E = max(abs(r[1].errmax - r[0].errmax), abs(r[-1].errmax - r[0].errmax))
    assert abs(err - r[0].errmax) <= 2.0 * E + 8.0 * np.spacing(r[0].errmax), (err, r[0].errmax, E)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the two kernels alone, on seeded random fields
KSHAPES = [(13, 9, 1031), (17, 11, 21), (9, 7, 1100), (16, 12, 28)]


def _inner(sz):
    return (slice(3, sz[1] + 1), slice(3, sz[0] + 1), slice(3, sz[2] + 1))  # 1-based 2..size-1 at padded index i + 1 (guide 2)


def _dot_bound(t):
    t = t.astype(np.float64).ravel()
    n = t.size
    mu = (n - 1) * 2.0 ** -53
    return math.fsum(t), mu / (1.0 - mu) * math.fsum(np.abs(t))


def _setup_kernel(prec, sz):
    from cubez_amd import CzHip
    h = CzHip(prec)
    R = h.real
    idx = np.array([2, sz[0] - 1, 2, sz[1] - 1, 2, sz[2] - 1], dtype=np.int32)
    scal = h.alloc((4, 4, 4), np.zeros((8, 8, 8), dtype=R))    # REAL scalars on the device
    dots = h.alloc((4, 4, 4), np.zeros((8, 8, 8), dtype=R))    # (read as doubles)
    return h, R, idx, scal, dots


def _dots_of(dots):
    return dots.get().view(np.float64).ravel()


@pytest.mark.parametrize("sz", KSHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_cg_update_kernel(prec, sz):
    h, R, idx, scal, dots = _setup_kernel(prec, sz)
    k = O.Kernels("oracle", prec)
    rng = np.random.default_rng(11)
    shape = (sz[1] + 4, sz[0] + 4, sz[2] + 4)
    x, r, p, q = (rng.standard_normal(shape).astype(R) for _ in range(4))
    alpha = R(0.37)
    s = np.zeros((8, 8, 8), dtype=R)
    s.ravel()[:2] = (alpha, -alpha)
    scal.put(s)
    dx, dr, dp, dq = (h.alloc(sz, a) for a in (x, r, p, q))
    f = h.lib.czhip_cg_update_async
    f.argtypes = [C.c_void_p] * 5 + [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_void_p]
    (_, szp), (_, idxp) = h._i(sz), h._i(idx)
    f(dx.ptr, dr.ptr, dp.ptr, dq.ptr, scal.ptr, szp, idxp, 2, dots.ptr)
    h.sync()
    xe, re_ = x.copy(), r.copy()
    k.blas_triad(xe, p, xe, alpha, list(sz), list(idx))
    k.blas_triad(re_, q, re_, R(-alpha), list(sz), list(idx))
    assert dx.get().tobytes() == xe.tobytes() and dr.get().tobytes() == re_.tobytes()
    S, B = _dot_bound(np.multiply(re_[_inner(sz)], re_[_inner(sz)], dtype=R))
    assert abs(_dots_of(dots)[0] - S) <= B, (_dots_of(dots)[0], S, B)


@pytest.mark.parametrize("first", [False, True], ids=["beta", "copy"])
@pytest.mark.parametrize("sz", KSHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_cg_dir_ax_kernel(prec, sz, first):
    h, R, idx, scal, dots = _setup_kernel(prec, sz)
    k = O.Kernels("oracle", prec)
    rng = np.random.default_rng(13)
    shape = (sz[1] + 4, sz[0] + 4, sz[2] + 4)
    inner = _inner(sz)
    z, pold = np.zeros(shape, dtype=R), np.zeros(shape, dtype=R)  # the shells are zero (what the kernel requires)
    z[inner] = rng.standard_normal(z[inner].shape)
    pold[inner] = rng.standard_normal(pold[inner].shape)
    pnew0, q0 = rng.standard_normal(shape).astype(R), rng.standard_normal(shape).astype(R)  # outside the inner box: must stay
    beta = R(-0.61)
    s = np.zeros((8, 8, 8), dtype=R)
    s.ravel()[2] = beta
    scal.put(s)
    dz, dpo, dpn, dq = (h.alloc(sz, a) for a in (z, pold, pnew0, q0))
    cf = np.array([1, 1, 1, 1, 1, 1, 6], dtype=R)
    f = h.lib.czhip_cg_dir_ax_async
    f.argtypes = [C.c_void_p] * 5 + [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p]
    (_, szp), (_, idxp), (cfa, cfp) = h._i(sz), h._i(idx), h._r(cf)
    beta_ptr = None if first else scal.ptr + 2 * np.dtype(R).itemsize
    f(dpn.ptr, dq.ptr, dz.ptr, dpo.ptr, beta_ptr, szp, idxp, 2, cfp, dots.ptr)
    h.sync()
    u = np.zeros(shape, dtype=R)
    if first:
        k.blas_copy(u, z, list(sz))
    else:
        k.blas_triad(u, pold, z, beta, list(sz), list(idx))  # u = R(beta*p_old) + z
    qe, pne = q0.copy(), pnew0.copy()
    k.blas_calc_ax(qe, u, list(sz), list(idx), cf)
    pne[inner] = u[inner]
    assert dpn.get().tobytes() == pne.tobytes(), "p_new"
    assert dq.get().tobytes() == qe.tobytes(), "q"
    assert dz.get().tobytes() == z.tobytes() and dpo.get().tobytes() == pold.tobytes()
    S, B = _dot_bound(np.multiply(u[inner], qe[inner], dtype=R))
    assert abs(_dots_of(dots)[0] - S) <= B, (_dots_of(dots)[0], S, B)


# ---------------------------------------------------------------------------------------------------------------------------------------------
def _cli(args, cwd):
    exe = os.path.join(ROOT, "cubez_amd", "cz_f64")
    return subprocess.run([exe] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=300)


def test_cli_pcg_refuses_asymmetric_preconditioner(tmp_path):
    p = _cli([32, 32, 32, "pcg", 100, 1.5, "sor2sma"], tmp_path)
    assert p.returncode == 0 and "Invalid preconditioner for pcg 'sor2sma' (none | jacobi)" in p.stdout, p.stdout
    assert "Iter =" not in p.stdout


def test_cli_pcg_refuses_jacobi_coefficient_out_of_range(tmp_path):
    p = _cli([32, 32, 32, "pcg", 100, 1.5, "jacobi"], tmp_path)
    assert p.returncode == 0 and "Invalid coefficient for pcg with jacobi" in p.stdout, p.stdout
    assert "Iter =" not in p.stdout


def test_cli_pcg_run(tmp_path):
    """the history file pcg.txt and the method lines"""
    p = _cli([32, 32, 32, "pcg", 500, 0.8, "jacobi"], tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Iterative Mehtod = PCG" in p.stdout and "Preconditioner = JACOBI" in p.stdout
    o = CP.run((32, 32, 32), 500, 0.8, "jacobi", prec="f64")
    assert f"Iter = {o.itr} " in p.stdout, p.stdout
    lines = (tmp_path / "pcg.txt").read_text().splitlines()
    assert lines[0].startswith("Itration") and len(lines) == o.itr + 1
