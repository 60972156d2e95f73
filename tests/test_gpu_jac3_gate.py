"""GPU tests (-m gpu) of the gated division of the three-sweep Jacobi pass (jac3_k, GATE = 1): whether a numerator is huge -- so large that the
division scales the divisor, |n| >= 2^(exponent(d) + 96), + 768 in FP64 -- is tested once per vector and wave; a wave without one divides by the
tail without that case, any other wave by the ungated form.  The gated tail is taken only for a divisor whose quotients were compared with
`n / d` on the context (czhip_selftest_gateddiv), gives the fields and residual sums of the ungated form bit for bit, also where both tails
run in one launch, and has an off switch (czhip_set_jac3_gate)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import special_operands as S  # noqa: E402

pytestmark = pytest.mark.gpu

OMG = 0.9
# from test_gpu_jac3_forms.BOXES: a row of 64 elements, rows of 128 (k windows by the rule), a box that does not start at 2, long rows
BOXES = [((40, 36, 60), None), ((33, 70, 124), None), ((24, 20, 28), (1, 24, 1, 20, 1, 28)), ((31, 23, 507), None), ((9, 7, 1100), None)]
BOX_IDS = [f"{b[0][0]}x{b[0][1]}x{b[0][2]}{'' if b[1] is None else '_idx'}" for b in BOXES]
FORMS3 = [(0, 0), (5, 0), (0, 3)]  # (vectors per k window, planes per chunk), as tests/test_gpu_special_operands.py
# (precision, jac3_medium): FP32 with the medium and with the hoisted division, FP64 (hoisted)
DIVISIONS = [("f32", 1), ("f32", 0), ("f64", 1)]
DIV_IDS = ["f32_medium", "f32_hoisted", "f64"]


def _hip(prec):
    from cubez_amd import CzHip
    h = CzHip(prec)
    h.lib.czhip_selftest_gateddiv.restype = C.c_longlong
    h.lib.czhip_selftest_gateddiv.argtypes = [h.creal, C.POINTER(C.c_longlong)]
    h.lib.czhip_jac3_division.argtypes = [h.creal]
    h.lib.czhip_jac3_gated.argtypes = [h.creal]
    return h


def _selftest(h, d):
    n = C.c_longlong(-7)
    bad = h.lib.czhip_selftest_gateddiv(d, C.byref(n))
    return bad, n.value


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_gated_division_selftest(prec):
    """Every numerator that is not huge, NaNs included: the gated tail gives the bits of `n / d`.  `compared` is a condition, not a
    measurement: at least 3/4 of the 2^32 numerators must have been compared.
    FP32, d = 6 or 6.2 (exponent 2): huge are the biased exponents 127 + 2 + 96 = 225 .. 254 and the infinities (the NaNs of 255 are
    compared): less than 31/256 = 12.1 % of all floats are left out.
    FP64: the sample is every one of the 4096 sign/exponent patterns x 2^20 mantissas; huge are the biased exponents 1023 + 2 + 768 =
    1793 .. 2046 and the infinities: less than 255/2048 = 12.5 % of the sample is left out."""
    h = _hip(prec)
    floor = 3 * (1 << 32) // 4
    if prec == "f32":
        for medium in (1, 0):  # the tail of the medium form and of the hoisted form
            assert h.lib.czhip_set_jac3_medium(medium) >= 0
            try:
                for d in (6.0, 6.2):
                    bad, n = _selftest(h, d)
                    print(f"f32 medium={medium} d={d}: {bad} differ of {n} compared")
                    assert bad == 0 and floor <= n <= (1 << 32), (medium, d, bad, n)
                assert _selftest(h, 3.0e38) == (-1, 0)
            finally:
                h.lib.czhip_set_jac3_medium(1)
    else:
        bad, n = _selftest(h, 6.0)
        print(f"f64 d=6: {bad} differ of {n} compared")
        assert bad == 0 and floor <= n <= (1 << 32), (bad, n)
        assert _selftest(h, 1.0e300) == (-1, 0)


def _coef(R, unit, rng):
    if unit:
        return np.array([1, 1, 1, 1, 1, 1, 6], dtype=R)
    cf = rng.uniform(0.5, 1.5, 7).astype(R)
    cf[6] = 6.2
    return cf


def _run_forms(h, sz, idx, p, b, cf, medium, gates=(1, 0)):
    """{(form, gate): (launched, field bytes, bytes of the three residual sums)} of jac3_k in every form of FORMS3"""
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    out = {}
    try:
        h.lib.czhip_set_jac3_medium(medium)
        for form in FORMS3:
            assert h.lib.czhip_set_jac3(2, *form) == 0
            for gate in gates:
                h.lib.czhip_set_jac3_gate(gate)
                assert h.tuning()["jac3_gate"] == gate
                # the form the launch takes: without this a verdict that quietly came out "not gated" would compare one kernel with itself
                assert h.lib.czhip_jac3_gated(float(cf[6])) == gate, (form, gate)
                dw = h.alloc(sz, p)
                ok, *rs = h.jacobi3(du, dw, db, sz, idx, cf, OMG)
                out[form, gate] = (ok, dw.get(), np.array(rs, dtype=np.float64).tobytes())
                dw.free()
        assert du.get().tobytes() == p.tobytes(), "the input field was modified"
    finally:
        h.lib.czhip_set_jac3_gate(1)
        h.lib.czhip_set_jac3_medium(1)
        h.lib.czhip_set_jac3(1, 0, 0)
        du.free(), db.free()
    return out


def _same_with_and_without_gate(out, nk, what, sums_of_nans=False):
    """field and residual sums bit for bit.  sums_of_nans: the fields hold NaNs of several payloads and signs, so a residual is a sum of
    different NaNs, and which of two NaN operands an addition hands on depends on the order the compiler gave the operands of that
    (commutative) addition -- it differs between the two instantiations (v_add_f64 acc, x against x, acc in their listings).  Such a sum
    must be NaN in both; every other sum, and every field value with its payload, keeps its bits."""
    for form in FORMS3:
        g, u = out[form, 1], out[form, 0]
        assert g[0] and u[0], (what, form, "the launcher declined")  # (every box of BOXES launches with czhip_set_jac3(2, ...), rows of 32 elements included)
        if g[0]:
            assert g[1].tobytes() == u[1].tobytes(), (what, form, "field")
            if sums_of_nans:
                gs, us = np.frombuffer(g[2], dtype=np.float64), np.frombuffer(u[2], dtype=np.float64)
                nan = np.isnan(us)
                assert (np.isnan(gs) == nan).all() and gs[~nan].tobytes() == us[~nan].tobytes(), (what, form, "residual sums", gs, us)
            else:
                assert g[2] == u[2], (what, form, "residual sums")


@pytest.mark.parametrize("unit", [0, 1], ids=["coef", "unit"])
@pytest.mark.parametrize("division", DIVISIONS, ids=DIV_IDS)
@pytest.mark.parametrize("box", BOXES, ids=BOX_IDS)
def test_gated_form_gives_the_bits_of_the_ungated_form(box, division, unit):
    """ordinary fields: output field and the three residual sums with czhip_set_jac3_gate(1) against (0), bit for bit"""
    prec, medium = division
    h = _hip(prec)
    (ni, nj, nk), idx = box
    sz = [ni, nj, nk]
    idx = list(idx) if idx else [2, ni - 1, 2, nj - 1, 2, nk - 1]
    rng = np.random.default_rng(7 * ni + 3 * nj + 13 * nk + unit)
    cf = _coef(h.real, unit, rng)
    p, b = (rng.uniform(-1, 1, (nj + 4, ni + 4, nk + 4)).astype(h.real) for _ in range(2))
    _same_with_and_without_gate(_run_forms(h, sz, idx, p, b, cf, medium), nk, (box, division, unit))


def _planted(prec, shape, d, rng):
    """(p, b): the `mixed` family of tests/special_operands.py (zeros, subnormals, tiny and ordinary values) with a few cells of p and of b
    replaced by 2^100 d, -2^120 (FP64: 2^772 d, -2^900: huge numerators for their neighbours and for themselves), +-inf, NaN (with a
    payload), -0.0, a subnormal and 2^-120 (2^-1000).  The cells lie in two rows i of two planes j and in a handful of k positions: a
    wave of jac3_k holds 64 consecutive vectors of the (i, k) plane, so most waves of a workgroup -- every other row band, every other k
    window -- meet no huge numerator and take the gated tail, while the waves around the planted cells take the general one, in every
    stage (the values spread by one cell per sweep)."""
    R = np.float32 if prec == "f32" else np.float64
    U = np.uint32 if prec == "f32" else np.uint64
    hi1, hi2, lo = (100, 120, -120) if prec == "f32" else (772, 900, -1000)
    nan = np.array([0x7fc12345 if prec == "f32" else 0x7ff8000012345678], dtype=U).view(R)[0]
    sub = np.array([0x00012345], dtype=U).view(R)[0]
    vals = [R(np.ldexp(float(d), hi1)), R(-np.ldexp(1.0, hi2)), R(np.inf), R(-np.inf), nan, R(-0.0), sub, R(np.ldexp(1.0, lo))]
    p, b = S.family("mixed", rng, shape, prec), S.family("mixed", rng, shape, prec)
    nj, ni, nk = shape
    js, is_ = sorted({3, nj // 2}), sorted({4, ni - 5})
    ks = sorted({3, 9, nk // 2, nk - 6})
    n = 0
    for arr in (p, b):
        for j in js:
            for i in is_:
                for k in ks:
                    arr[j, i, k] = vals[n % len(vals)]
                    n += 1
    return p, b


def _three_single_sweeps(h, sz, idx, p, b, cf):
    """three launches of the single-sweep entry (stencil_k, the plain n / d)"""
    dp, db, dw = h.alloc(sz, p), h.alloc(sz, b), h.alloc(sz, np.zeros_like(p))
    try:
        res = [h.jacobi(dp, sz, idx, cf, OMG, db, dw) for _ in range(3)]
        return dp.get(), res
    finally:
        dp.free(), db.free(), dw.free()


@pytest.mark.parametrize("unit", [0, 1], ids=["coef", "unit"])
@pytest.mark.parametrize("division", DIVISIONS, ids=DIV_IDS)
@pytest.mark.parametrize("box", BOXES, ids=BOX_IDS)
def test_both_tails_in_one_launch(box, division, unit):
    """Fields with huge, infinite, NaN, zero, subnormal and tiny cells planted so that some waves of a workgroup hold a huge numerator and
    others none: the field gated against ungated bit for bit, NaN payloads included (the residual sums: _same_with_and_without_gate); and against three single sweeps: NaNs in the same places, every
    other value bit for bit (which payload a sum of two NaNs carries depends on the operand order the compiler chose in either kernel, and
    IEEE 754 leaves it open; the gated and the ungated pass are the same kernel source but for the division, and are held to the payload)."""
    prec, medium = division
    h = _hip(prec)
    (ni, nj, nk), idx = box
    sz = [ni, nj, nk]
    idx = list(idx) if idx else [2, ni - 1, 2, nj - 1, 2, nk - 1]
    rng = np.random.default_rng(5 * ni + 11 * nj + 17 * nk + unit)
    cf = _coef(h.real, unit, rng)
    p, b = _planted(prec, (nj + 4, ni + 4, nk + 4), cf[6], rng)
    out = _run_forms(h, sz, idx, p, b, cf, medium)
    _same_with_and_without_gate(out, nk, (box, division, unit), sums_of_nans=True)
    want, want_res = _three_single_sweeps(h, sz, idx, p, b, cf)
    assert np.isnan(want).any() and np.isinf(want).any(), "the planted cells did not reach the result"
    for form in FORMS3:
        ok, got, res = out[form, 1]
        assert ok, (box, division, unit, form, "the launcher declined")
        nan = np.isnan(want)
        assert (np.isnan(got) == nan).all(), (box, division, unit, form, "NaNs in other places")
        U = f"u{got.itemsize}"
        assert (got.view(U)[~nan] == want.view(U)[~nan]).all(), (box, division, unit, form, "field against three single sweeps")
        for g, w in zip(np.frombuffer(res, dtype=np.float64), want_res):
            assert (np.isnan(g) and np.isnan(w)) or g == w or abs(g - w) <= 1e-11 * abs(w), (box, division, unit, form, g, w)


def test_switch():
    """czhip_set_jac3_gate returns the setting that was in force, negative keeps it, czhip_tuning_describe shows it; a divisor outside
    fastdiv_ok is still refused by the pass whatever the switch says"""
    h = _hip("f32")
    assert h.lib.czhip_set_jac3_gate(0) == 1
    try:
        assert h.tuning()["jac3_gate"] == 0
        assert h.lib.czhip_set_jac3_gate(-1) == 0
        assert h.tuning()["jac3_gate"] == 0
    finally:
        assert h.lib.czhip_set_jac3_gate(1) == 0
    assert h.tuning()["jac3_gate"] == 1
    for d in (3.0e38, -3.0e38, 1.0e-30):
        assert h.lib.czhip_jac3_division(d) == -1, d
    assert h.lib.czhip_jac3_division(6.0) == 1  # (the gate does not change what czhip_jac3_division reports: 1 medium, 0 hoisted)
    assert h.lib.czhip_jac3_gated(6.0) == 1 and h.lib.czhip_jac3_gated(3.0e38) == -1
    assert h.lib.czhip_set_jac3_gate(0) == 1
    try:
        assert h.lib.czhip_jac3_gated(6.0) == 0
    finally:
        h.lib.czhip_set_jac3_gate(1)
    h64 = _hip("f64")
    assert h64.tuning()["jac3_gate"] == 1
    assert h64.lib.czhip_jac3_division(1.0e300) == -1 and h64.lib.czhip_jac3_division(6.0) == 0
