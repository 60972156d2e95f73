"""GPU tests (-m gpu) of the division forms of the three-sweep Jacobi pass (jac3_k): the shorter FP32 division (mediumdiv, one correction step)
is taken only for a divisor whose 2^32 quotients were compared with `n / d` on the context and agreed in every bit, gives the fields and
residuals of the hoisted form, and has an off switch (czhip_set_jac3_medium, CZHIP_JAC3_MEDIUM)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the boxes of the two-stage pass tests (test_gpu_kernels.T2_BOXES)
BOXES = [((40, 36, 60), None), ((33, 70, 124), None), ((130, 20, 252), None), ((70, 45, 124), None),
         ((24, 20, 28), (1, 24, 1, 20, 1, 28)), ((64, 9, 60), None), ((96, 40, 508), None),
         ((40, 36, 61), None), ((33, 50, 123), None), ((70, 20, 126), None), ((29, 31, 253), None),
         ((24, 20, 59), (1, 24, 1, 20, 1, 59)), ((31, 23, 507), None),
         ((9, 7, 1100), None), ((7, 6, 2100), None)]


def _hip(prec):
    from cubez_amd import CzHip
    h = CzHip(prec)
    h.lib.czhip_selftest_mediumdiv.restype = C.c_longlong
    h.lib.czhip_selftest_mediumdiv.argtypes = [h.creal]
    h.lib.czhip_jac3_division.argtypes = [h.creal]
    return h


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_medium_division_selftest(prec):
    """The exhaustive comparison of the shorter division with `n / d`: no differing numerator for the benchmark's 6 and the tests' 6.2 (FP32);
    -1 for a divisor outside fastdiv_ok and in FP64, which has no such form."""
    h = _hip(prec)
    if prec == "f32":
        assert h.lib.czhip_selftest_mediumdiv(6.0) == 0
        assert h.lib.czhip_selftest_mediumdiv(6.2) == 0
        assert h.lib.czhip_selftest_mediumdiv(3.0e38) == -1
    else:
        assert h.lib.czhip_selftest_mediumdiv(6.0) == -1


@pytest.mark.parametrize("unit", [0, 1], ids=["coef", "unit"])
@pytest.mark.parametrize("box", BOXES, ids=[f"{b[0][0]}x{b[0][1]}x{b[0][2]}{'' if b[1] is None else '_idx'}" for b in BOXES])
def test_medium_form_gives_the_bits_of_the_hoisted_form(box, unit):
    """jac3_k FP32 with the shorter division and with the hoisted one: the same output field and the same three residual sums, bit for bit."""
    h = _hip("f32")
    (ni, nj, nk), idx = box
    sz = [ni, nj, nk]
    idx = list(idx) if idx else [2, ni - 1, 2, nj - 1, 2, nk - 1]
    rng = np.random.default_rng(3 * ni + 5 * nj + 11 * nk + unit)
    shape = (nj + 4, ni + 4, nk + 4)
    if unit:
        cf = np.array([1, 1, 1, 1, 1, 1, 6], dtype=np.float32)
    else:
        cf = rng.uniform(0.5, 1.5, 7).astype(np.float32)
        cf[6] = 6.2
    p, b = (rng.uniform(-1, 1, shape).astype(np.float32) for _ in range(2))
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    out = {}
    try:
        assert h.lib.czhip_set_jac3(2, -1, -1) == 0
        for med in (1, 0):
            h.lib.czhip_set_jac3_medium(med)
            assert h.lib.czhip_jac3_division(float(cf[6])) == med
            dw = h.alloc(sz, p)
            ok, r1, r2, r3 = h.jacobi3(du, dw, db, sz, idx, cf, 0.9)
            out[med] = (ok, dw.get().tobytes(), (r1, r2, r3))
            dw.free()
    finally:
        h.lib.czhip_set_jac3_medium(1)
        h.lib.czhip_set_jac3(1, -1, -1)
        du.free(), db.free()
    assert out[1][0] == out[0][0]
    if out[1][0]:
        assert out[1][1] == out[0][1]
        assert out[1][2] == out[0][2]
    if nk + 4 >= 64:
        assert out[1][0]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_divisor_outside_fastdiv_ok_never_takes_the_medium_form(prec):
    """A divisor near the ends of the exponent range: the pass does not take it at all (-1), so neither form of its division runs; FP64 never
    takes the shorter form."""
    h = _hip(prec)
    big, tiny = (3.0e38, 1.0e-30) if prec == "f32" else (1.0e300, 1.0e-300)
    for d in (big, -big, tiny):
        assert h.lib.czhip_jac3_division(d) == -1, d
    sz, idx = [40, 36, 60], [2, 39, 2, 35, 2, 59]
    R = np.float32 if prec == "f32" else np.float64
    cf = np.array([1, 1, 1, 1, 1, 1, big], dtype=R)
    p = np.zeros((36 + 4, 40 + 4, 60 + 4), dtype=R)
    du, dw, db = h.alloc(sz, p), h.alloc(sz, p), h.alloc(sz, p)
    try:
        h.lib.czhip_set_jac3(2, -1, -1)
        ok, *_ = h.jacobi3(du, dw, db, sz, idx, cf, 0.9, probe=1)
        assert not ok
    finally:
        h.lib.czhip_set_jac3(1, -1, -1)
        du.free(), dw.free(), db.free()
    if prec == "f64":
        assert h.lib.czhip_jac3_division(6.0) == 0


def test_off_switch():
    """czhip_set_jac3_medium(0) and CZHIP_JAC3_MEDIUM=0 (read when a thread's context starts) keep the hoisted division."""
    h = _hip("f32")
    assert h.lib.czhip_set_jac3_medium(0) == 1
    try:
        assert h.lib.czhip_jac3_division(6.0) == 0
        assert h.lib.czhip_set_jac3_medium(-1) == 0
    finally:
        assert h.lib.czhip_set_jac3_medium(1) == 0
    assert h.lib.czhip_jac3_division(6.0) == 1

    got = {}

    def fresh_context():
        try:
            got["env"] = h.lib.czhip_jac3_division(6.0)
        except Exception as e:  # pragma: no cover - reported below
            got["err"] = repr(e)

    os.environ["CZHIP_JAC3_MEDIUM"] = "0"
    try:
        t = threading.Thread(target=fresh_context)
        t.start()
        t.join()
    finally:
        os.environ.pop("CZHIP_JAC3_MEDIUM")
    assert got == {"env": 0}
