"""Face coefficients for pcg on the GPU (-m gpu), through the public interface only, every result against the numpy
restatement of tests/coef_parity.py: the operator (cz_get_residual) and cz_sub_grad byte for byte in every layout the coefficients come in,
PCG against the exact-dot restatement, CZ.project end to end in the six states, clearing, the refusals, the stream hand-over, Refined."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coef_parity as K  # noqa: E402
import periodic_parity as P  # noqa: E402
import problem_parity as PP  # noqa: E402
import project_parity as J  # noqa: E402
import test_gpu_neumann as TN  # noqa: E402
from test_gpu_periodic import _handle  # noqa: E402
from test_gpu_problem import _real, _torch  # noqa: E402
from test_gpu_project import KEEP, OUTSIDE, SCALE, _back, _on, _placed  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = [(9, 7, 12), (33, 47, 61), (3, 40, 40), (40, 40, 1100)]
SHAPE_IDS = ["x".join(map(str, g)) for g in SHAPES]
SOLVER = ["pcg", 50, 1.2, "mgrb"]
# the layouts the coefficients come in: (layout of tests/test_gpu_project.py, device tensors or numpy, the import's kernel form)
COEF_LAYOUTS = [("c_order", True, 1), ("c_order", False, 1), ("slice", True, 1), ("interleaved", False, 3), ("interleaved", True, 3)]


def _set_coef(cz, layout, dev, gsz, R, beta, torch):
    bases, views = _placed(layout, gsz, R, beta)
    held = _on(torch if dev else None, bases)
    cz.set_face_coef(*views(held))
    assert cz.info()["face_coef"] == 1
    return held


def _check_operator(cz, prec, gsz, name, torch):
    """set_rhs(0), set_field(p), get_residual = -A p byte for byte, the sum to 1e-12 and the same bits twice; then sub_grad with sentinels"""
    R, state = _real(prec), K.STATES[name]
    _, p = PP.problem(gsz, prec, 1)
    beta = K.random(gsz, prec, 1)
    zero = np.zeros(gsz, dtype=R)
    want, ss_ref = K.residual(J.fill_field(p, state), zero, beta, state)
    for layout, dev, form in COEF_LAYOUTS:
        what = (gsz, name, prec, layout, dev)
        _set_coef(cz, layout, dev, gsz, R, beta, torch)
        assert cz.info()["field_form"] == form, what
        cz.set_rhs(zero)
        cz.set_field(p)
        got, ss = cz.get_residual(dtype=R)
        assert got.tobytes() == want.tobytes(), what
        assert abs(ss - ss_ref) <= 1e-12 * ss_ref, (what, ss, ss_ref)
        out = torch.empty(gsz, dtype=getattr(torch, np.dtype(R).name), device="cuda")
        _, ss2 = cz.get_residual(out=out)
        assert ss2 == ss and out.cpu().numpy().tobytes() == want.tobytes(), what
        assert cz.get_residual()[1] == ss, what
        cz.set_face_coef(None)
        assert cz.info()["face_coef"] == 0
    return beta, p


def _check_grad(cz, prec, gsz, name, torch, layout, form, beta, p):
    R, state = _real(prec), K.STATES[name]
    vel = J.velocity(gsz, prec, 1)
    for a, m in zip(vel, J.written(gsz, state[1])):
        a[~m] = KEEP
    cz.set_field(p)
    bases, views = _placed(layout, gsz, R, vel)
    dev = _on(torch, bases)
    cz.sub_grad(*views(dev), scale=SCALE)
    assert cz.info()["field_form"] == form, (layout, cz.info()["field_form"])
    new = K.sub_grad(vel, J.fill_field(p, state), beta, state[1], SCALE, R)
    want, _ = _placed(layout, gsz, R, new)
    for a, b in zip(_back(dev), want):
        assert a.tobytes() == b.tobytes(), (gsz, name, prec, layout, form)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", SHAPES, ids=SHAPE_IDS)
def test_operator_and_gradient_bytes(gsz, prec):
    """the six states where the box allows: -A p through get_residual with the coefficients from every layout, then sub_grad in the row form
    (device, C order and a slice with odd phases) and the generic form (an interleaved numpy array)"""
    torch = _torch()
    for name in K.STATES:
        if not J.fits(gsz, K.STATES[name]):
            continue
        cz = _handle(prec, list(gsz) + SOLVER, K.STATES[name])
        try:
            beta, p = _check_operator(cz, prec, gsz, name, torch)
            cz.set_face_coef(*beta)
            _check_grad(cz, prec, gsz, name, torch, "c_order", 1, beta, p)
            _check_grad(cz, prec, gsz, name, torch, "slice", 1, beta, p)
            _check_grad(cz, prec, gsz, name, None, "interleaved", 3, beta, p)
        finally:
            cz.close()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_gradient_bytes_with_the_generic_form_forced(prec, monkeypatch):
    """CZ_FIELD_FORM=3: the generic kernels (import of the coefficients, gradient) on the layouts the row form takes otherwise"""
    torch = _torch()
    monkeypatch.setenv("CZ_FIELD_FORM", "3")
    for gsz in SHAPES[:3]:
        for name in ("dirichlet", "channel"):
            if not J.fits(gsz, K.STATES[name]):
                continue
            cz = _handle(prec, list(gsz) + SOLVER, K.STATES[name])
            try:
                R = _real(prec)
                beta = K.random(gsz, prec, 1)
                _, p = PP.problem(gsz, prec, 1)
                cz.set_face_coef(*beta)
                assert cz.info()["field_form"] == 3
                want, _ = K.residual(J.fill_field(p, K.STATES[name]), np.zeros(gsz, dtype=R), beta, K.STATES[name])
                cz.set_rhs(np.zeros(gsz, dtype=R))
                cz.set_field(p)
                assert cz.get_residual(dtype=R)[0].tobytes() == want.tobytes()
                _check_grad(cz, prec, gsz, name, torch, "c_order", 3, beta, p)
                _check_grad(cz, prec, gsz, name, None, "slice", 3, beta, p)
            finally:
                cz.close()


# ---- PCG against the exact-dot restatement
@pytest.mark.parametrize("c", K.PCG_CASES, ids=[c["id"] for c in K.PCG_CASES])
def test_pcg_against_the_exact_dot_restatement(c):
    """K iterations: FP32 bit for bit (field and history), FP64 within 2 E + 8 ulp with the history within its envelope
    (tests/test_coef_oracle.py holds the premise of every case); the counters"""
    torch = _torch()
    gsz, prec, state = c["gsz"], c["prec"], K.STATES[c["state"]]
    b, p, beta = K.case_problem(c)
    cz = _handle(prec, list(gsz) + ["pcg", c["K"], c["coef"], c["pc"]], state)
    try:
        cz.set_eps(1e-30)
        cz.set_face_coef(*[torch.from_numpy(a).cuda() for a in beta])
        cz.set_rhs(b)
        cz.set_field(p)
        itr = cz.solve()
        got, hist, info = cz.field(), cz.history(), cz.info()
    finally:
        cz.close()
    assert itr == c["K"] and info["face_coef"] == 1 and info["cg_fused"] == 0
    if c["pc"] in ("mg", "mgrb"):
        assert info["mg_cycles"] == c["K"]
    if prec == "f32":
        ref = K.case_run(c)
        assert got.tobytes() == ref.P.tobytes(), c["id"]
        assert hist == [v for _, v in ref.history], c["id"]
    else:
        ref, E, Eh = K.envelope_f64(gsz, c["pc"], c["coef"], state, c["K"], b, p, beta, eps=1e-30)
        ok, worst = PP.f64_close(got, ref.P, E)
        assert ok, (c["id"], worst)
        okh, worsth = PP.f64_close(hist, [v for _, v in ref.history], Eh)
        assert okh, (c["id"], worsth)


# ---- CZ.project end to end
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", list(K.STATES))
@pytest.mark.parametrize("gsz", K.E2E_BOXES, ids=["x".join(map(str, g)) for g in K.E2E_BOXES])
def test_project_end_to_end(gsz, name, prec):
    """pcg mgrb 1.2 and mg 0.8 at eps 1e-10 (FP32: 1e-5) with smooth(4) and bubble(10): a second set_rhs_div gives ||div||_2 / ||div before||_2
    within coef_parity.BARS (8 x the restatement's ratio), the count within 1 of the restatement's"""
    torch = _torch()
    state = K.STATES[name]
    vel = J.velocity(gsz, prec, 0, state)
    _, p0 = PP.problem(gsz, prec, 0)
    for pc, coef in K.E2E_RUNS:
        cz = _handle(prec, list(gsz) + ["pcg", 300, coef, pc], state)
        try:
            cz.set_eps(J.E2E_EPS[prec])
            for field in K.E2E_FIELDS:
                cz.set_face_coef(*K.FIELDS[field](gsz, prec))
                cz.set_field(p0)
                t = [torch.from_numpy(a).cuda() for a in vel]
                itr, ss0 = cz.project(*t)
                ss1 = cz.set_rhs_div(*t)
                ratio, (ref_ratio, ref_itr) = math.sqrt(ss1 / ss0), K.MEASURED[tuple(gsz), pc, field, name, prec]
                print(f"{gsz} {name} {prec} {pc} {field}: ratio {ratio:.3e} (restatement {ref_ratio:.3e}, bar {K.BARS[name, prec]:.3e})  itr {itr} (restatement {ref_itr})")
                assert 0 < itr < 300 and ratio <= K.BARS[name, prec], (pc, field, ratio, K.BARS[name, prec])
                assert abs(itr - ref_itr) <= 1, (pc, field, itr, ref_itr)
                assert cz.info()["face_coef"] == 1 and cz.info()["cg_fused"] == 0
        finally:
            cz.close()


# ---- clearing
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["dirichlet", "inflow"])
def test_cleared_handle_gives_the_bytes_of_a_twin(name, prec):
    """after set_face_coef(None), and after a second setup, a solve gives the field, the history and cg_fused of a handle that never had
    coefficients"""
    gsz, state = (33, 47, 61), K.STATES[name]
    b, p = PP.problem(gsz, prec, 2)
    args = list(gsz) + ["pcg", 6, 1.2, "mgrb"]

    def solved(cz):
        cz.set_eps(1e-30)
        cz.set_rhs(b)
        cz.set_field(p)
        return cz.solve(), cz.field().tobytes(), cz.history(), cz.info()["cg_fused"], cz.info()["face_coef"]

    twin = _handle(prec, args, state)
    try:
        want = solved(twin)
    finally:
        twin.close()
    assert want[0] == 6 and want[4] == 0 and want[3] == (6 if name == "dirichlet" else 0)
    cz = _handle(prec, args, state)
    try:
        cz.set_face_coef(*K.random(gsz, prec))
        with_coef = solved(cz)
        assert with_coef[4] == 1 and with_coef[3] == 0 and with_coef[1] != want[1]
        cz.set_face_coef(None)
        assert solved(cz) == want
        cz.set_face_coef(*K.random(gsz, prec))
        assert cz.setup(args) == 1  # a set-up clears the coefficients as it clears the masks
        assert cz.info()["face_coef"] == 0
        if name != "dirichlet":
            cz.set_neumann(state[0])
        assert solved(cz) == want
    finally:
        cz.close()


# ---- the refusals
def _raw(cz, arrs, strides, on_device=0):
    ptr = [C.c_void_p(a) if a is not None else None for a in arrs]
    st = (C.c_longlong * 3)(*strides) if strides is not None else None
    return cz.lib.cz_set_face_coef(cz.h, *ptr, st, on_device, None)


def _state_bytes(cz, gsz, R):
    """P and (through the residual of P) the right-hand side, as bytes"""
    return cz.field().tobytes(), cz.get_residual(dtype=R)[0].tobytes()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_refusals(prec, capfd):
    from cubez_amd import CZ
    gsz, R = (9, 7, 12), _real(prec)
    beta = K.random(gsz, prec)
    ptrs = [a.ctypes.data for a in beta]
    st = [s // beta[0].itemsize for s in beta[0].strides]
    n = 0
    fresh = CZ(prec, quiet=True)
    try:
        assert _raw(fresh, ptrs, st) == 0  # before cz_setup
        n += 1
    finally:
        fresh.close()
    cz = _handle(prec, list(gsz) + SOLVER)
    try:
        b0, p0 = PP.problem(gsz, prec, 4)
        cz.set_rhs(b0)
        cz.set_field(p0)
        before = _state_bytes(cz, gsz, R)
        cases = [([None, ptrs[1], ptrs[2]], st, 0), ([ptrs[0], ptrs[1], None], st, 0), ([None, None, ptrs[2]], st, 0),  # some but not all NULL
                 (ptrs, None, 0), (ptrs, [0, st[1], st[2]], 0), (ptrs, [st[0], -st[1], st[2]], 0),  # a NULL stride, a stride < 1
                 ([ptrs[0], ptrs[1] + 1, ptrs[2]], st, 0),  # misaligned
                 (ptrs, st, 1)]  # not memory of the device
        for arrs, strides, on_dev in cases:
            assert _raw(cz, arrs, strides, on_dev) == 0, (arrs, strides, on_dev)
            n += 1
            assert cz.info()["face_coef"] == 0
        with pytest.raises(ValueError):
            cz.set_face_coef(beta[0], beta[1], np.asfortranarray(beta[2]))  # unequal strides
        with pytest.raises(ValueError):
            cz.set_face_coef(beta[0], beta[1], None)
        assert _state_bytes(cz, gsz, R) == before
        # a refusal of the first kind leaves coefficients that are in force alone
        cz.set_face_coef(*beta)
        assert _raw(cz, [None, ptrs[1], ptrs[2]], st) == 0 and cz.info()["face_coef"] == 1
        n += 1
        # a bad value on a face that is read: refused, and the handle is left WITHOUT coefficients
        for v in (0.0, -1.0, math.inf, math.nan):
            for ax, at in ((0, (0, 3, 4)), (1, (2, 5, 4)), (2, (3, 2, 10))):
                bad = [a.copy() for a in beta]
                bad[ax][at] = v
                cz.set_face_coef(*beta)
                with pytest.raises(RuntimeError):
                    cz.set_face_coef(*bad)
                n += 1
                assert cz.info()["face_coef"] == 0, (v, ax)
        # the same values where the operator does not read: accepted, and nothing changes
        cz.set_face_coef(*beta)
        want = cz.get_residual(dtype=R)[0].tobytes()
        for v in (0.0, -1.0, math.inf, math.nan):
            odd = [np.where(m, R(v), a) for a, m in zip(beta, K.unread(gsz, (0, 0, 0)))]
            cz.set_face_coef(*odd)
            assert cz.info()["face_coef"] == 1 and cz.get_residual(dtype=R)[0].tobytes() == want, v
        cz.set_face_coef(None)
        assert _state_bytes(cz, gsz, R) == before
    finally:
        cz.close()
    maf = _handle(prec, list(gsz) + ["jacobi_maf", 50, 0.8])
    try:
        assert _raw(maf, ptrs, st) == 0
        n += 1
    finally:
        maf.close()
    other = _handle(prec, list(gsz) + ["sor2sma", 50, 1.5])  # accepted on a handle of any other solver, which then refuses to solve
    try:
        keep = other.field().tobytes()
        assert _raw(other, ptrs, st) == 1 and other.info()["face_coef"] == 1
        assert other.solve() == 0 and other.sweeps(2) == 0 and other.field().tobytes() == keep
        other.set_face_coef(None)
        assert other.solve() > 0
    finally:
        other.close()
    err = capfd.readouterr().err
    assert err.count("cz_set_face_coef:") == n, err
    assert err.count("face coefficients are set (cz_set_face_coef) and the solver is not pcg") == 2, err
    for why in ("cz_setup first", "all three arrays", "NULL pointer", "strides must be positive", "not aligned", "handle's device",
                "not finite and positive", "left without coefficients", "MAF"):
        assert why in err, why


def test_periodic_face_one_is_ignored_and_a_later_periodic_call_is_followed():
    """periodic X: NaN on face 1 of bx is accepted (face n - 1 is read in its place); coefficients set BEFORE set_periodic give the bytes of
    coefficients set after it, and going back to Dirichlet faces reads face 1's own value again"""
    gsz, prec, R = (9, 7, 12), "f64", np.float64
    beta = K.random(gsz, prec)
    _, p = PP.problem(gsz, prec, 1)
    zero = np.zeros(gsz, dtype=R)
    nanned = [a.copy() for a in beta]
    nanned[0][0] = np.nan
    want_px, _ = K.residual(J.fill_field(p, K.STATES["px"]), zero, nanned, K.STATES["px"])
    want_d, _ = K.residual(p, zero, beta, K.STATES["dirichlet"])
    cz = _handle(prec, list(gsz) + SOLVER)
    try:
        cz.set_rhs(zero)
        cz.set_face_coef(*beta)
        cz.set_periodic((1, 0, 0))
        cz.set_field(p)
        assert cz.info()["face_coef"] == 1 and cz.get_residual(dtype=R)[0].tobytes() == want_px.tobytes()
        cz.set_face_coef(*nanned)
        assert cz.get_residual(dtype=R)[0].tobytes() == want_px.tobytes()
        cz.set_face_coef(*beta)
        cz.set_periodic((0, 0, 0))
        cz.set_field(p)
        assert cz.info()["face_coef"] == 1 and cz.get_residual(dtype=R)[0].tobytes() == want_d.tobytes()
    finally:
        cz.close()


def test_a_decomposed_run_is_refused(capfd):
    """(2, 1, 1) on the LOCAL transport: the entry returns 0 on every rank, with the line that names the follow-up"""
    gsz = (32, 36, 40)

    def work(q):
        cz = _handle("f32", list(gsz) + ["pcg", 10, 0.8, "jacobi", 2, 1, 1])
        try:
            beta = [np.ones(tuple(cz.local()["size"]), dtype=np.float32) for _ in range(3)]
            before = cz.field()
            out = _raw(cz, [a.ctypes.data for a in beta], [s // 4 for s in beta[0].strides])
            return out, cz.info()["face_coef"], cz.field().tobytes() == before.tobytes()
        finally:
            cz.close()

    assert TN._ranks("f32", (2, 1, 1), work) == [(0, 0, True)] * 2
    err = capfd.readouterr().err
    assert err.count("cz_set_face_coef: a decomposed run") == 2 and err.count("follow-up") == 2, err


# ---- the stream hand-over
def test_stream_hand_over():
    """coefficients produced on a side stream right before the call and overwritten right after it: the solve is that of a twin"""
    torch = _torch()
    gsz, prec, state = (64, 64, 64), "f64", K.STATES["inflow"]
    beta = K.smooth(gsz, prec, 4)
    b, p = PP.problem(gsz, prec, 3)
    args = list(gsz) + ["pcg", 5, 1.2, "mgrb"]

    def solved(cz):
        cz.set_eps(1e-30)
        cz.set_rhs(b)
        cz.set_field(p)
        return cz.solve(), cz.field().tobytes(), cz.history()

    twin = _handle(prec, args, state)
    try:
        twin.set_face_coef(*beta)
        want = solved(twin)
    finally:
        twin.close()
    cz = _handle(prec, args, state)
    try:
        s = torch.cuda.Stream()
        host = [torch.from_numpy(a).pin_memory() for a in beta]
        junk = torch.empty(256 * 1024 * 1024 // 8, dtype=torch.float64, device="cuda")
        src = [torch.empty(gsz, dtype=torch.float64, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(8):
                junk.fill_(1.0)  # work in front of the final values, on the caller's stream
            for a, h in zip(src, host):
                a.fill_(-1.0)
                a.copy_(h, non_blocking=True)
            cz.set_face_coef(*src)
            for a in src:
                a.fill_(float("nan"))  # the caller may reuse its arrays at once
        assert solved(cz) == want
    finally:
        cz.close()


# ---- Refined
def test_refined_with_coefficients():
    """smooth(4) at 64^3 reaches 1e-10; the outer steps are within 1 of the restatement's refinement with the coefficient kernels"""
    import refine_parity as RP
    from cubez_amd.refine import Refined
    _torch()
    gsz, state = (64, 64, 64), K.STATES["dirichlet"]
    beta = K.smooth(gsz, "f64", 4)
    b, p = PP.problem(gsz, "f64", 0)
    r = Refined(gsz)
    try:
        r.set_face_coef(*beta)
        assert r.hi.info()["face_coef"] == 1 and r.lo.info()["face_coef"] == 1
        r.set_rhs(b)
        r.set_field(p)
        steps = r.solve(tol=1e-10)
        hist = list(r.history)
        r.set_face_coef(None)
        assert r.hi.info()["face_coef"] == 0 and r.lo.info()["face_coef"] == 0
    finally:
        r.close()
    assert steps > 0 and hist[-1][1] <= 1e-10, hist
    # the restatement: periodic_parity.refine's loop with the coefficient kernels (FP64 residual, FP32 inner solve on the rounded coefficients)
    beta32 = [a.astype(np.float32) for a in beta]
    npts = int(np.prod([n - 2 for n in gsz]))
    q = p.astype(np.float64).copy()
    ss0 = K.residual(q, b, beta, state)[1]
    ss, ref_steps = ss0, 0
    while True:
        scale = RP.scale_of(ss, npts)
        res, ss = K.residual(q, b, beta, state)
        if math.sqrt(ss) <= 1e-10 * math.sqrt(ss0) or ref_steps == 20:
            break
        r32 = RP.scaled(res, scale, np.float32)
        o = K.run(list(gsz), "mgrb", 1.2, "f32", state, 1000, r32, np.zeros(gsz, dtype=np.float32), beta32, eps=RP.INNER_EPS)
        q = RP.add(q, PP.unpad(o.P), 1.0 / scale)
        ref_steps += 1
    print("outer steps", steps, "restatement", ref_steps, hist)
    assert abs(steps - ref_steps) <= 1
