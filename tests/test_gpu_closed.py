"""The closed box for pcg on the GPU (-m gpu), every result against the restatement of tests/closed_parity.py: shift_sums_k
and the closed form of cg_update_k alone; PCG iteration by iteration (CZ_MG_TAIL 1 and 0); the V-cycles with mask 63; a solve to
convergence on an incompatible right-hand side; decomposed runs on the LOCAL transport; a manufactured zero-mean solution; mixed-precision
refinement; refusals and state."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_parity as CB  # noqa: E402
import mg_parity as M  # noqa: E402
import neumann_parity as N  # noqa: E402
import problem_parity as PP  # noqa: E402
import test_gpu_neumann as TN  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
G = O.GUIDE
OMG = TN.OMG


def _handle(prec, args, closed=True):
    from cubez_amd import CZ
    cz = CZ(prec, quiet=True)
    assert cz.setup(list(args)) == 1
    if closed:
        cz.set_closed_box(True)
    return cz


# ---- the two kernels alone
KERNEL_BOXES = [(9, 7, 12), (33, 47, 61), (6, 5, 1030)]  # (6, 5, 1030): long rows, vector tails, every phase of a row against the vector width


def kernel_field(gsz, prec):
    """(a, m): a padded array full of seeded random numbers (every cell: the kernel must leave those outside the inner box alone), a shift"""
    R = np.float32 if prec == "f32" else np.float64
    a = np.random.default_rng(31).standard_normal((gsz[1] + 2 * G, gsz[0] + 2 * G, gsz[2] + 2 * G)).astype(R)
    return a, R(0.0123456789)


def shift_terms(a, m, gsz):
    """the terms of the kernel's two sums: a' = a - m over the inner box (m None: a), and the REAL products a' a'"""
    sz, idx = TN._box(gsz)
    v = a[M.inner(sz, idx)]
    if m is not None:
        v = v - m
    return v.astype(np.float64), np.multiply(v, v, dtype=a.dtype).astype(np.float64)


def _small(hip, values=()):
    s = np.zeros((8, 8, 8), dtype=hip.real)
    s.ravel()[:len(values)] = values
    return hip.alloc((4, 4, 4), s)


def _doubles(d):
    return d.get().view(np.float64).ravel()


@pytest.mark.parametrize("shift", [False, True], ids=["sums", "shift"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", KERNEL_BOXES, ids=["x".join(map(str, g)) for g in KERNEL_BOXES])
def test_shift_sums_kernel(gsz, prec, shift):
    """the inner box takes a - m (one REAL subtraction) or stays (m NULL); every byte outside it stays; the sums within gamma_64 sum|t| of
    the correctly rounded ones, and in FP32 the same REALs (tests/test_closed_oracle.py::test_kernel_case_premise)"""
    from cubez_amd.lib import CzHip
    hip = CzHip(prec)
    sz, idx = TN._box(gsz)
    a, m = kernel_field(gsz, prec)
    d, dm, sums = hip.alloc(sz, a), _small(hip, [m]), _small(hip)
    try:
        hip.timing(True)
        assert hip.shift_sums(d, dm if shift else None, sz, idx, sums)
        hip.sync()
        want = a.copy()
        ins = M.inner(sz, idx)
        if shift:
            want[ins] = want[ins] - m
            assert not np.array_equal(want, a)
        assert d.get().tobytes() == want.tobytes()
        got = _doubles(sums)[:2]
        for g, t in zip(got, shift_terms(a, m if shift else None, gsz)):
            S, B = CB.sum_bound(t)
            print(f"shift_sums {gsz} {prec} shift={shift}: gpu {g!r} exact {S!r} bound {B:.3e}")
            assert abs(g - S) <= B, (g, S, B)
            if prec == "f32":
                assert np.float32(g) == np.float32(S)
        assert hip.timing_read("shift_sums")[0] == 1
    finally:
        hip.timing(False)
        hip.sync()
        for x in (d, dm, sums):
            x.free()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", KERNEL_BOXES, ids=["x".join(map(str, g)) for g in KERNEL_BOXES])
def test_cg_update_closed_kernel(gsz, prec):
    """x = alpha p + x, r = ((-alpha) q + r) - m by the oracle's blas_triad and one subtraction, byte for byte; r.r and sum r within their bounds"""
    from cubez_amd.lib import CzHip
    hip = CzHip(prec)
    R = hip.real
    sz, idx = TN._box(gsz)
    k = O.Kernels("oracle", prec)
    shape = (gsz[1] + 2 * G, gsz[0] + 2 * G, gsz[2] + 2 * G)
    rng = np.random.default_rng(11)
    x, r, p, q = (rng.standard_normal(shape).astype(R) for _ in range(4))
    alpha, m = R(0.37), R(-3.21e-4)
    sc, dots = _small(hip, [alpha, -alpha, 0, 0, m]), _small(hip)
    dev = [hip.alloc(sz, v) for v in (x, r, p, q)]
    try:
        hip.cg_update_closed(*dev, sc, sz, idx, dots)
        hip.sync()
        xe, re_ = x.copy(), r.copy()
        k.blas_triad(xe, p, xe, alpha, list(sz), list(idx))
        k.blas_triad(re_, q, re_, R(-alpha), list(sz), list(idx))
        ins = M.inner(sz, idx)
        re_[ins] = re_[ins] - m
        assert dev[0].get().tobytes() == xe.tobytes() and dev[1].get().tobytes() == re_.tobytes()
        assert dev[2].get().tobytes() == p.tobytes() and dev[3].get().tobytes() == q.tobytes()
        got = _doubles(dots)[:2]
        Ssq, Bsq = CB.sum_bound(np.multiply(re_[ins], re_[ins], dtype=R))
        Ss, Bs = CB.sum_bound(re_[ins])
        assert abs(got[0] - Ssq) <= Bsq and abs(got[1] - Ss) <= Bs, (got, Ssq, Bsq, Ss, Bs)
    finally:
        hip.sync()
        for v in dev + [sc, dots]:
            v.free()


def _means_close(c, g, o, E=None):
    """closed_mean 0 and 2 against the restatement: FP32 the same REALs; FP64 within closed_parity.mean_tol, the mean of x also within what
    the field's own bar (2 E + 8 ulp) lets its mean move"""
    if c["prec"] == "f32":
        assert g["means"][0] == float(o.means[0]) and g["means"][2] == float(o.means[2]), (g["means"], o.means)
        return
    assert abs(g["means"][0] - float(o.means[0])) <= o.mean_tol[0], (g["means"], o.means, o.mean_tol)
    slack = 0.0 if E is None else 2.0 * float(E.max()) + 8.0 * float(np.spacing(np.abs(o.P).max() + abs(float(o.means[2]))))
    assert abs(g["means"][2] - float(o.means[2])) <= o.mean_tol[2] + slack, (g["means"], o.means, o.mean_tol, slack)


# ---- PCG, K iterations against the exact-dot restatement
def _pcg_gpu(c, b, p, itr_max, eps, division=None, closed=True):
    cz = _handle(c["prec"], list(c["gsz"]) + ["pcg", itr_max, c["coef"], c["pc"]] + (list(division) if division else []), closed=False)
    try:
        cz.timing(True)
        if closed:
            cz.set_closed_box(True)
        cz.set_rhs(b)
        cz.set_field(p)
        cz.set_eps(eps)
        itr = cz.solve()
        return dict(itr=itr, hist=list(cz.history()), P=cz.field(), X=cz.get_field(), info=cz.info(), launches=cz.launches(),
                    means=[cz.closed_mean(w) for w in range(3)])
    finally:
        cz.timing(False)
        cz.close()


@pytest.mark.parametrize("tail", [1, 0])
@pytest.mark.parametrize("c", CB.CASES, ids=[c["id"] for c in CB.CASES])
def test_pcg_iterations_vs_exact_dot_restatement(c, tail, monkeypatch):
    """FP32: count, history and the whole padded field bit for bit; FP64: within 2 E + 8 ulp (problem_parity.f64_close).  The closed update
    is cg_update_k's closed form every iteration; no fused pair runs"""
    monkeypatch.setenv("CZ_MG_TAIL", str(tail))
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    g = _pcg_gpu(c, b, p, c["K"], 1e-30)
    if c["prec"] == "f32":
        o, E, Eh = CB.case_run(c), None, None
    else:
        o, E, Eh = CB.envelope_f64(c["gsz"], c["pc"], c["coef"], c["K"], b, p, eps=1e-30)
    TN._close(c, g, o, E, Eh)
    assert g["X"].tobytes() == PP.unpad(g["P"]).tobytes()
    L = g["launches"]
    # (two passes each: the built-in right-hand side when the mode went on, the caller's b, the initial residual, the answer)
    assert L["cg_update_closed"] == c["K"] and L["shift_sums"] == 8, L
    assert L["bc_mirror"] > 0 and L["jacobi2"] == L["jacobi3"] == L["rbsor2"] == L["rbsor4"] == 0, L
    assert g["info"]["neumann"] == 63 and g["info"]["closed"] == 1 and g["info"]["cg_fused"] == 0
    _means_close(c, g, o, E)
    if c["pc"] in ("mg", "mgrb"):
        assert g["info"]["mg_cycles"] == c["K"]
        if tail == 0:
            assert L["mg_tail"] == 0, L


@pytest.mark.parametrize("fuse", ["0", "1"])
def test_the_closed_update_does_not_follow_cg_fuse(fuse, monkeypatch):
    monkeypatch.setenv("CZ_CG_FUSE", fuse)
    c = CB.CASES[2]
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    g = _pcg_gpu(c, b, p, c["K"], 1e-30)
    TN._close(c, g, CB.case_run(c), None, None)
    assert g["launches"]["cg_update_closed"] == c["K"]


# ---- the V-cycles with mask 63
CYCLE_BOXES = [(9, 7, 12), (33, 47, 61), (3, 40, 40)]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", CYCLE_BOXES, ids=["x".join(map(str, g)) for g in CYCLE_BOXES])
def test_precondition_with_six_faces_equals_the_restatement(gsz, prec):
    sz, idx, ins, r = TN._cycle_rhs(prec, gsz)
    for kind in ("mg", "mgrb"):
        k = N.Kernels("oracle", prec)
        k.faces = CB.SIX
        ref = N.apply(kind, k, r, sz, idx, OMG[kind], CB.SIX)[ins]
        cz = _handle(prec, list(gsz) + ["pcg", 1, OMG[kind], kind])
        try:
            z = cz.precondition(r)[ins]
            assert cz.info()["neumann"] == 63
        finally:
            cz.close()
        assert np.isfinite(z).all() and z.tobytes() == ref.tobytes(), kind


# ---- to convergence on the incompatible seeded right-hand side
@pytest.mark.parametrize("pc,coef", CB.COUNT_RUNS, ids=[f"{a}_{w}" for a, w in CB.COUNT_RUNS])
def test_to_convergence_on_an_incompatible_rhs(pc, coef):
    """33 x 47 x 61 FP64 eps 1e-5: the restatement's count, the restatement's mean of b, an answer of zero mean within
    closed_parity.mean_bound"""
    c = dict(gsz=CB.COUNT_BOX, prec="f64", pc=pc, coef=coef, id=f"count_{pc}")
    b, p = PP.problem(c["gsz"], "f64", 0)
    g = _pcg_gpu(c, b, p, 300, 1e-5)
    o = CB.run(c["gsz"], pc, coef, "f64", 300, b, p, eps=1e-5)
    assert g["itr"] == o.itr == CB.COUNTS[pc, coef], (g["itr"], o.itr)
    assert g["hist"][-1] < 1e-5
    assert abs(g["means"][0] - float(o.means[0])) <= o.mean_tol[0], (g["means"], o.means, o.mean_tol)
    x = g["X"][1:-1, 1:-1, 1:-1]
    mean = math.fsum(x.ravel()) / x.size
    bound = CB.mean_bound(g["means"][2], np.abs(x).max(), np.float64)
    print(f"closed {pc}: mean of the answer {mean:.3e}, bound {bound:.3e}, means {g['means']}")
    assert abs(mean) <= bound, (mean, bound)


# ---- decomposed runs on the LOCAL transport
@pytest.mark.parametrize("c,div", CB.DECOMP, ids=[d[0]["id"] for d in CB.DECOMP])
def test_decomposed_solve(c, div):
    """the gathered field of a decomposed solve under the bar of the existing decomposed tests: FP32 bit for bit, FP64 within the envelope"""
    gsz, prec = c["gsz"], c["prec"]
    b, p = PP.problem(gsz, prec, 0)
    X = np.full(gsz, np.nan, dtype=b.dtype)

    def work(q):
        cz = _handle(prec, list(gsz) + ["pcg", 100, c["coef"], c["pc"]] + list(div))
        try:
            sl = cz.global_slice()
            cz.set_rhs(b[sl])
            cz.set_field(p[sl])
            itr = cz.solve()
            cz.get_field(X[sl])
            return itr, list(cz.history()), cz.info(), [cz.closed_mean(w) for w in range(3)]
        finally:
            cz.close()

    out = TN._ranks(prec, div, work)
    assert all(o[0] == out[0][0] and o[1] == out[0][1] and o[3] == out[0][3] for o in out)
    assert all(o[2]["closed"] == 1 and o[2]["neumann"] == 63 for o in out)
    if prec == "f32":
        o, E, Eh = CB.run(gsz, c["pc"], c["coef"], prec, 100, b, p), None, None
    else:
        o, E, Eh = CB.envelope_f64(gsz, c["pc"], c["coef"], 100, b, p)
    assert o.res < O.EPS and o.itr < 100
    TN._close(c, dict(itr=out[0][0], hist=out[0][1], P=PP.pad(X)), o, E, Eh)
    _means_close(c, dict(means=out[0][3]), o, E)


# ---- a manufactured zero-mean solution
def test_manufactured_zero_mean_solution_pcg_mgrb_64_f64():
    """64^3 FP64, pcg 100 1.0 mgrb, eps 1e-10: a smooth zero-mean u, b = N u by the oracle.  The bar of
    test_gpu_neumann.py::test_manufactured_solution_pcg_mgrb_64_f64: the GPU's max error against u is at most the restatement's plus
    2 E + 8 ulp"""
    gsz = (64, 64, 64)
    u, b = CB.manufactured(gsz)
    p = np.zeros(gsz)
    c = dict(gsz=gsz, prec="f64", pc="mgrb", coef=1.0, id="manufactured")
    g = _pcg_gpu(c, b, p, 100, 1e-10)
    r = {q: CB.run(gsz, "mgrb", 1.0, "f64", 100, b, p, eps=1e-10, perturb=q) for q in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr == g["itr"] < 100
    ui = u[1:-1, 1:-1, 1:-1]
    err = {q: float(np.abs(PP.unpad(r[q].P)[1:-1, 1:-1, 1:-1] - ui).max()) for q in r}
    E = max(abs(err[1] - err[0]), abs(err[-1] - err[0]))
    gerr = float(np.abs(g["X"][1:-1, 1:-1, 1:-1] - ui).max())
    print("manufactured (closed box): restated error", err[0], "GPU error", gerr, "envelope", E, "iterations", g["itr"])
    assert gerr <= err[0] + 2.0 * E + 8.0 * np.spacing(np.abs(u).max())


# ---- mixed-precision refinement
def test_refined_closed_reaches_1e10_in_the_restated_steps():
    from test_gpu_problem import _torch
    _torch()
    import refine_parity as RP
    from cubez_amd.refine import Refined
    gsz = (33, 47, 61)
    b, p = PP.problem(gsz, "f64", 0)
    want, hist, _, ratios = CB.refine(b, p, tol=1e-10)
    assert want > 0 and ratios[-1] <= 1e-10 and RP.premise(ratios, 1e-10, int(np.prod([n - 2 for n in gsz])))
    with pytest.raises(ValueError):
        Refined(gsz, closed=True, neumann=N.FIVE)
    R = Refined(gsz, closed=True)
    try:
        R.set_rhs(b)
        R.set_field(p)
        steps = R.solve(tol=1e-10)
        x = R.get_field()
        assert steps == want, (steps, R.history, hist)
        assert R.history[-1][1] <= 1e-10 and [h[2] for h in R.history] == [h[2] for h in hist]
        assert R.hi.info()["closed"] == R.lo.info()["closed"] == 1 and R.hi.info()["neumann"] == 63
        assert np.array_equal(x[0, 1:-1, 1:-1], x[1, 1:-1, 1:-1]) and np.array_equal(x[1:-1, 1:-1, -1], x[1:-1, 1:-1, -2])
    finally:
        R.close()


def test_refinement_steps_through_host_arrays():
    """the loop of cubez_amd.refine.Refined written with host arrays (no torch): an FP64 handle that never solves, an FP32 pcg 1000 1.2 mgrb,
    the mode on both; 1e-10 in the restated loop's outer steps, with its inner iteration counts"""
    import refine_parity as RP
    from cubez_amd.refine import INNER_EPS, scale_of
    gsz = (33, 47, 61)
    b, p = PP.problem(gsz, "f64", 0)
    want, hist, _, ratios = CB.refine(b, p, tol=1e-10)
    npts = int(np.prod([n - 2 for n in gsz]))
    assert want > 0 and ratios[-1] <= 1e-10 and RP.premise(ratios, 1e-10, npts)
    hi = _handle("f64", list(gsz) + ["jacobi", 1, 0.8])
    lo = _handle("f32", list(gsz) + ["pcg", 1000, 1.2, "mgrb"])
    try:
        hi.set_rhs(b)
        hi.set_field(p)
        _, ss0 = hi.get_residual()
        ss, steps, got = ss0, 0, []
        while True:
            scale = scale_of(ss, npts)
            r32, ss = hi.get_residual(dtype=np.float32, scale=scale)
            if math.sqrt(ss) <= 1e-10 * math.sqrt(ss0) or steps == 20:
                break
            lo.set_rhs(r32)
            lo.set_field(np.zeros(gsz, dtype=np.float32))
            lo.set_eps(INNER_EPS)
            inner = lo.solve()
            assert inner > 0
            hi.add_field(lo.get_field(), 1.0 / scale)
            steps += 1
            got.append(inner)
        assert steps == want and got == [h[2] for h in hist], (steps, got, hist)
        x = hi.get_field()
        assert np.array_equal(x[0, 1:-1, 1:-1], x[1, 1:-1, 1:-1]) and np.array_equal(x[1:-1, 1:-1, -1], x[1:-1, 1:-1, -2])
    finally:
        hi.close()
        lo.close()


# ---- refusals and state
def test_refusals_and_state(capfd):
    from cubez_amd import CZ
    six = (C.c_int * 6)
    cz = CZ("f32", quiet=True)
    try:
        assert cz.lib.cz_set_closed_box(cz.h, 1) == 0  # before cz_setup
        assert math.isnan(cz.closed_mean(3)) and math.isnan(cz.closed_mean(-1))
        assert cz.setup([9, 7, 12, "jacobi", 50, 0.8]) == 1
        assert cz.info()["closed"] == 0
        assert cz.lib.cz_set_neumann(cz.h, six(1, 1, 1, 1, 1, 1)) == 0 and cz.info()["neumann"] == 0  # six flags: still refused
        cz.set_closed_box(True)  # accepted on a handle of another solver, which then refuses to solve and leaves P alone
        assert cz.info()["closed"] == 1 and cz.info()["neumann"] == 63
        before = cz.field()
        assert cz.solve() == 0 and cz.sweeps(4) == 0 and cz.evaluate([9, 7, 12, "jacobi", 50, 0.8]) == 0
        assert cz.field().tobytes() == before.tobytes() and cz.info()["closed"] == 1
        cz.set_neumann(N.Z_BOTH)  # an accepted cz_set_neumann leaves the mode
        assert cz.info()["closed"] == 0 and cz.info()["neumann"] == N.bits(N.Z_BOTH)
        cz.set_closed_box(True)
        cz.set_closed_box(False)
        assert cz.info()["closed"] == 0 and cz.info()["neumann"] == 0
        assert cz.solve() > 0
    finally:
        cz.close()
    err = capfd.readouterr().err
    assert err.count("cz_set_closed_box:") == 1 and err.count("cz_set_neumann:") == 1 and "cz_set_closed_box" in err.split("cz_set_neumann:")[1]
    assert err.count("cz_solve:") == 1 and err.count("cz_sweeps:") == 1 and err.count("cz_evaluate:") == 1, err
    maf = CZ("f32", quiet=True)
    try:
        assert maf.setup([9, 7, 12, "jacobi_maf", 50, 0.8]) == 1
        assert maf.lib.cz_set_closed_box(maf.h, 1) == 0 and maf.info()["closed"] == 0
        with pytest.raises(ValueError):
            maf.set_closed_box(True)
        assert maf.solve() > 0
    finally:
        maf.close()
    assert capfd.readouterr().err.count("cz_set_closed_box:") == 2


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_rhs_mean_survives_every_call_that_uses_the_scalars(prec, monkeypatch):
    """The mean that set_rhs removes on a closed box stays on the device until closed_mean(0) asks for it (the one member of the driver's
    device scalars that lives across calls; it used to land in a different double in each precision).  Handle A asks at
    once.  The B handles make the same two calls from the same device array, then every call a pcg handle accepts that touches the
    scalars, and ask last: the same kernel on the same input, so the same bits, without a tolerance.  A handle's preconditioner and
    CZ_CG_FUSE are fixed when it is made, so the second solve (none, CZ_CG_FUSE=0) has a handle of its own"""
    from test_gpu_problem import _torch
    torch = _torch()
    gsz = (9, 7, 12)
    b, p = PP.problem(gsz, prec, 5)
    bd = torch.from_numpy(b).cuda()
    ones = [np.ones(gsz, dtype=b.dtype) for _ in range(3)]

    def start(pc):
        cz = _handle(prec, list(gsz) + ["pcg", 3, 1.0, pc])
        cz.set_rhs(bd)
        return cz

    a = start("mgrb")
    try:
        want = a.closed_mean(0)
    finally:
        a.close()
    assert want != 0.0 and math.isfinite(want)

    b1 = start("mgrb")
    try:
        b1.set_field(p)
        b1.set_eps(1e-30)
        assert b1.solve() == 3  # (cut at three iterations)
        assert b1.get_residual()[1] > 0.0
        b1.set_face_coef(*ones)
        assert b1.info()["face_coef"] == 1 and b1.get_residual()[1] > 0.0
        b1.set_face_coef(None)
        sz, idx, ins, r = TN._cycle_rhs(prec, gsz)
        assert np.isfinite(b1.precondition(r)[ins]).all()
        got = [b1.closed_mean(w) for w in range(3)]
    finally:
        b1.close()
    assert got[0] == want and math.isfinite(got[1]) and math.isfinite(got[2]), (got, want)

    monkeypatch.setenv("CZ_CG_FUSE", "0")
    b2 = start("none")
    try:
        b2.set_field(p)
        b2.set_eps(1e-30)
        assert b2.solve() == 3
        got = [b2.closed_mean(w) for w in range(3)]
    finally:
        b2.close()
    assert got[0] == want and math.isfinite(got[1]) and math.isfinite(got[2]), (got, want)


def test_setup_clears_the_mode_and_off_gives_the_unmasked_bits():
    """cz_setup (through cz_evaluate) after the mode: the unmasked solve of a fresh handle; on = 0 after on = 1: a Dirichlet solve of the
    caller's problem with the bits of a handle that never saw the mode, given the projected right-hand side"""
    from cubez_amd import CZ
    ev, fresh = CZ("f64", quiet=True), CZ("f64", quiet=True)
    try:
        args = [9, 7, 12, "pcg", 100, 0.8, "mg"]
        assert ev.setup(args) == 1
        ev.set_closed_box(True)
        assert ev.evaluate(args) == 1 and ev.info()["closed"] == 0 and ev.info()["neumann"] == 0
        assert fresh.evaluate(args) == 1
        assert ev.iter == fresh.iter and ev.field().tobytes() == fresh.field().tobytes() and ev.info()["cg_fused"] == ev.iter
    finally:
        ev.close()
        fresh.close()
    gsz = (33, 47, 61)
    b, p = PP.problem(gsz, "f32", 0)
    args = list(gsz) + ["pcg", 100, 1.2, "mgrb"]
    a, plain = _handle("f32", args, closed=False), _handle("f32", args, closed=False)
    try:
        a.set_closed_box(True)
        a.set_rhs(b)
        a.set_closed_box(False)
        sz, idx = TN._box(gsz)
        B = PP.pad(b)
        m = CB.project(B, sz, idx)
        assert a.closed_mean(0) == float(m)
        plain.set_rhs(PP.unpad(B))
        for cz in (a, plain):
            cz.set_field(p)
        assert a.solve() == plain.solve() > 0
        assert a.field().tobytes() == plain.field().tobytes() and a.info()["cg_fused"] == a.iter
        assert a.closed_mean(0) != 0.0 and a.setup(args) == 1  # a new set-up: nothing was removed yet
        assert [a.closed_mean(w) for w in range(3)] == [0.0, 0.0, 0.0]
    finally:
        a.close()
        plain.close()
