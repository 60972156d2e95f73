"""GPU tests (-m gpu) of the plane step of the three-sweep Jacobi pass (jac3_k) where its forms meet: the first, inner and last steps of a
chunk's march (plane addresses carried from step to step and open plane gates against the clamped, gated general form), the masks of
partial vectors at every alignment of the box edge inside a component pair, and the FP32 update on zeros, subnormals and tiny values (the
cases a step with wave masks in scalar registers or packed FP32 operations has to pass; both were built, measured and not kept:
profiles/r19/jac3_step_instructions.txt).  Every case goes through czhip_jacobi3_async against three oracle sweeps: fields bit for bit, the
input untouched, the three residual sums to 1e-11; every listed form must be taken by the launcher."""
import os
import sys

import numpy as np
import pytest

from oracle import cz_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from special_operands import special  # noqa: E402

pytestmark = pytest.mark.gpu

OMG = 0.9
WHOLE = 1 << 20  # planes per chunk: more than any box here has -> one chunk for the whole box


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _coef(R, unit, rng):
    if unit:
        return np.array([1, 1, 1, 1, 1, 1, 6], dtype=R)
    cf = rng.uniform(0.5, 1.5, 7).astype(R)
    cf[6] = 6.2
    return cf


def _three_oracle_sweeps(ko, p, b, sz, idx, cf):
    a, w, r = p.copy(), np.zeros_like(p), []
    for _ in range(3):
        wide = np.zeros(1)
        ko.jacobi(a, sz, idx, cf, OMG, b, w, wide=wide)
        r.append(wide[0])
    return a, r


def _check_forms(h, p, b, sz, idx, cf, want, res, forms):
    """every (window, chunk) form: launched, output == want bit for bit, input untouched, residuals to 1e-11"""
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    try:
        for kw, tj in forms:
            assert h.lib.czhip_set_jac3(2, kw, tj) == 0
            dw = h.alloc(sz, p)
            try:
                ok, r1, r2, r3 = h.jacobi3(du, dw, db, sz, idx, cf, OMG)
                assert ok, (kw, tj, "the launcher declined")
                got = dw.get()
                if got.tobytes() != want.tobytes():
                    bad = np.argwhere(got.view(f"u{got.itemsize}") != want.view(f"u{got.itemsize}"))
                    print(f"form {(kw, tj)} idx {idx}: {len(bad)} points differ, first (j, i, k) = {bad[:8].tolist()}")
                assert got.tobytes() == want.tobytes(), (kw, tj, idx)
                assert du.get().tobytes() == p.tobytes(), (kw, tj)
                for got_r, want_r in zip((r1, r2, r3), res):
                    print(f"form {(kw, tj)} idx {idx}: residual sum {got_r!r} oracle {want_r!r} rel {_rel(got_r, want_r):.2e}")
                    assert _rel(got_r, want_r) < 1e-11, (kw, tj, got_r, want_r)
            finally:
                dw.free()
    finally:
        h.lib.czhip_set_jac3(1, 0, 0)
        du.free(), db.free()


# ---- 1. the ends of the march: boxes of 1, 2, 3, 4, 5, 9 inner planes (chunks shorter than the pipeline; the array's last plane is read) and
# a sub-box that touches neither the first nor the last plane of the array; chunks of 2, 3, 7 planes and one chunk for the whole box.  Last: a
# box whose j range ends at nj, one plane further than the default box and the furthest the pass takes: its last chunk requests the array's
# last plane, so its inner steps must stop one step early (the `jlast - 3` arm of jac3_k's `qi`)
MARCH = [(3, None), (4, None), (5, None), (6, None), (7, None), (11, None), (16, (4, 13)), (9, (2, 9))]
MARCH_FORMS = [(0, 2), (0, 3), (0, 7), (0, WHOLE)]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("nj,jr", MARCH, ids=[f"nj{nj}{'' if jr is None else '_sub'}" for nj, jr in MARCH])  # (nj9_sub: j = 2 .. nj)
def test_first_inner_and_last_steps_of_a_chunk(prec, nj, jr):
    from cubez_amd import CzHip
    ni, nk = 12, 28
    sz = [ni, nj, nk]
    idx = [2, ni - 1, 2, nj - 1, 2, nk - 1] if jr is None else [2, ni - 1, jr[0], jr[1], 2, nk - 1]
    h, ko = CzHip(prec), O.Kernels("oracle", prec)
    R = ko.real
    rng = np.random.default_rng(1000 + nj)
    cf = _coef(R, 1, rng)
    p, b = (rng.uniform(-1, 1, (nj + 4, ni + 4, nk + 4)).astype(R) for _ in range(2))
    want, res = _three_oracle_sweeps(ko, p, b, sz, idx, cf)
    _check_forms(h, p, b, sz, idx, cf, want, res, MARCH_FORMS)


# ---- 2. pairs and partial vectors: rows of 61 .. 64 elements, k ranges from 2 / 3 to nk - 1 / nk - 2 (every alignment of the box edge inside
# a component pair), windows of 5 vectors and whole rows
@pytest.mark.parametrize("unit", [0, 1], ids=["coef", "unit"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("nkp", [61, 62, 63, 64])
def test_box_edge_at_every_place_of_a_component_pair(nkp, prec, unit):
    from cubez_amd import CzHip
    ni, nj, nk = 10, 9, nkp - 4
    sz = [ni, nj, nk]
    h, ko = CzHip(prec), O.Kernels("oracle", prec)
    R = ko.real
    rng = np.random.default_rng(7 * nkp + unit)
    cf = _coef(R, unit, rng)
    p, b = (rng.uniform(-1, 1, (nj + 4, ni + 4, nk + 4)).astype(R) for _ in range(2))
    for k0 in (2, 3):
        for k1 in (nk - 1, nk - 2):
            idx = [2, ni - 1, 2, nj - 1, k0, k1]
            want, res = _three_oracle_sweeps(ko, p, b, sz, idx, cf)
            _check_forms(h, p, b, sz, idx, cf, want, res, [(5, 0), (0, 0)])


# ---- 3. values on which a packed FP32 operation, or a flushing one, would round unlike the single IEEE operation (the family `special` of
# tests/special_operands.py: it reaches the division's special branch in the first of the three stages; tests/test_gpu_special_operands.py has
# the families that reach it in every stage)
def test_update_on_zeros_subnormals_and_tiny_values():
    from cubez_amd import CzHip
    ni, nj, nk = 12, 10, 60
    sz, idx = [ni, nj, nk], [2, ni - 1, 2, nj - 1, 2, nk - 1]
    h, ko = CzHip("f32"), O.Kernels("oracle", "f32")
    rng = np.random.default_rng(20190)
    cf = np.array([1, 1, 1, 1, 1, 1, 6], dtype=np.float32)
    shape = (nj + 4, ni + 4, nk + 4)
    p, b = special(rng, shape), special(rng, shape)
    for x in (p, b):  # every class is present
        assert (x == 0).any() and np.signbit(x[x == 0]).any() and (np.abs(x) == np.float32(2.0 ** -149)).any()
        assert ((np.abs(x) > 0) & (np.abs(x) < np.float32(2.0 ** -126))).any() and ((np.abs(x) >= 2.0 ** -120) & (np.abs(x) <= 2.0 ** -100)).any()
    want, res = _three_oracle_sweeps(ko, p, b, sz, idx, cf)
    _check_forms(h, p, b, sz, idx, cf, want, res, [(0, 0), (5, 0), (0, 3)])
