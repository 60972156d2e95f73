"""GPU tests (-m gpu) of the plane step of the three-sweep Jacobi pass (jac3_k) with the LDS operands of the next stage requested while a
stage computes (cubez_amd/csrc/cz_k_jac3.h, "LDS in flight"): every wave requests the operands of all three stages, also a wave that skips a
stage, and holds a second set of six while the division of the stage before runs -- its out-of-line general tail included.  What can go
wrong is a value taken from the wrong set, from the wrong buffer parity or before it arrived, so the cases are the ones that change which
waves run which stage (whole rows of 31 .. 100 vectors, asked for with a window of that length and the planned geometry asserted: from 64 the
end waves only request stage 2's operands), where a wave's vectors lie in a k window, which steps take the inner and the general form
(chunks of 2 .. 10 planes), and which stage of a step leaves the straight-line path.  Every case goes through czhip_jacobi3_async against
three oracle sweeps: fields bit for bit, the input untouched, the three residual sums to 1e-11; every listed form must be taken by the
launcher."""
import os
import sys

import numpy as np
import pytest

from oracle import cz_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import special_operands as S  # noqa: E402

pytestmark = pytest.mark.gpu

OMG = 0.9
WHOLE = 1 << 20  # planes per chunk: more than any box here has -> one chunk for the whole box
VEC = {"f32": 4, "f64": 2}  # elements per vector


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _three_oracle_sweeps(ko, p, b, sz, idx, cf):
    a, w, r = p.copy(), np.zeros_like(p), []
    for _ in range(3):
        wide = np.zeros(1)
        ko.jacobi(a, sz, idx, cf, OMG, b, w, wide=wide)
        r.append(wide[0])
    return a, r


def _check_forms(h, p, b, sz, idx, cf, want, res, forms, nans=False):
    """every (window, chunk) form: launched, output == want bit for bit, input untouched, residuals to 1e-11.  nans: the fields hold NaNs and
    infinities -- a NaN must meet a NaN (IEEE 754 leaves open which payload a sum of two NaNs carries), every other value keeps its bits; a
    residual sum that is NaN or infinite in the oracle must be the same here"""
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    U = f"u{p.itemsize}"
    try:
        for kw, tj in forms:
            assert h.lib.czhip_set_jac3(2, kw, tj) == 0
            dw = h.alloc(sz, p)
            try:
                ok, r1, r2, r3 = h.jacobi3(du, dw, db, sz, idx, cf, OMG)
                assert ok, (kw, tj, "the launcher declined")
                got = dw.get()
                keep = ~np.isnan(want) if nans else np.ones(want.shape, dtype=bool)
                if nans:
                    assert (np.isnan(got) == np.isnan(want)).all(), (kw, tj, idx, "NaNs in other places")
                same = got.view(U)[keep] == want.view(U)[keep]
                if not same.all():
                    bad = np.argwhere(keep & (got.view(U) != want.view(U)))
                    print(f"form {(kw, tj)} idx {idx}: {len(bad)} points differ, first (j, i, k) = {bad[:8].tolist()}")
                assert same.all(), (kw, tj, idx)
                assert du.get().tobytes() == p.tobytes(), (kw, tj)
                for got_r, want_r in zip((r1, r2, r3), res):
                    print(f"form {(kw, tj)} idx {idx}: residual sum {got_r!r} oracle {want_r!r}")
                    if np.isfinite(want_r):
                        assert _rel(got_r, want_r) < 1e-11, (kw, tj, got_r, want_r)
                    else:
                        assert nans and ((np.isnan(got_r) and np.isnan(want_r)) or got_r == want_r), (kw, tj, got_r, want_r)
            finally:
                dw.free()
    finally:
        h.lib.czhip_set_jac3(1, 0, 0)
        du.free(), db.free()


def _geometry(prec, sz, idx, kwin):
    """(R, k windows, row segments per window) of the pass the launcher plans for this box (restated from launch_deep and plan_pass,
    cz_h_launch.h, as tests/test_gpu_jac3_flight.py does): 1024 vectors per workgroup, four halo rows.  Window 0 in czhip_set_jac3 is the
    launcher's own rule (26 / 36 vectors), NOT whole rows: whole rows of Rfull vectors are asked for with a window of Rfull"""
    v, hv = (4, 1) if prec == "f32" else (2, 2)
    rfull = -(-(sz[2] + 4) // v)
    want = kwin if kwin > 0 else (26 if v == 4 else 36)
    r, nwin = rfull, 1
    if rfull > want + 2 * hv:
        nwin = -(-rfull // want)
        r = -(-rfull // nwin) + 2 * hv
    assert r <= 128, "the launcher declines rows of more than 1024 / 8 vectors"
    rows = idx[1] - idx[0] + 1
    return r, nwin, -(-rows * r // (1024 - 4 * r))


def _case(prec, ni, nj, nk, forms, seed, idx=None, expect=None):
    """expect: {window: (R, k windows, row segments)} -- the shape the case is about, checked for every form with that window"""
    from cubez_amd import CzHip
    sz = [ni, nj, nk]
    idx = idx or [2, ni - 1, 2, nj - 1, 2, nk - 1]
    for kw, _ in forms:
        if expect is not None and kw in expect:
            assert _geometry(prec, sz, idx, kw) == expect[kw], (prec, sz, kw, _geometry(prec, sz, idx, kw), expect[kw])
    h, ko = CzHip(prec), O.Kernels("oracle", prec)
    rng = np.random.default_rng(seed)
    cf = S.coef(ko.real, 1)
    p, b = (rng.uniform(-1, 1, (nj + 4, ni + 4, nk + 4)).astype(ko.real) for _ in range(2))
    want, res = _three_oracle_sweeps(ko, p, b, sz, idx, cf)
    _check_forms(h, p, b, sz, idx, cf, want, res, forms)


# ---- 1. which waves run which stage.  A workgroup's 1024 threads hold the vectors of its segment +- two rows of R vectors; stage 2 is for the
# waves that hold a vector of the segment +- one row, stage 3 for those that own one.  Below R = 32 every wave runs all three; from 32 the
# first and the last wave own nothing; from 64 they hold no vector of stage 2's set either (wave2 false): they only request its operands, from
# addresses no running stage reads in those lanes, and publish v2 = v1 while that set is held.  WHOLE rows of R vectors: a window of R (the
# geometry is asserted: R, one window, two segments -- the skipping waves of one workgroup hold what the next one owns).  The forms with
# window 0 run the same boxes by the launcher's own rule (FP32: 2 .. 4 windows of 18 .. 27 vectors; FP64: whole rows up to 36, else 36 / 38).
ROWS = [(31, 40), (32, 40), (63, 16), (64, 16), (100, 10)]  # (R, ni)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("R,ni", ROWS, ids=[f"R{r}" for r, _ in ROWS])
def test_waves_that_skip_a_stage(R, ni, prec):
    _case(prec, ni, 12, VEC[prec] * R - 4, [(R, 3), (R, WHOLE), (0, 3), (0, WHOLE)], 3100 + R, expect={R: (R, 1, 2)})


# ---- 2. k windows: rows of 128 vectors in 26 windows of 5 and in 5 windows of 26 vectors (with the halo R = 7 / 9 and 28 / 30: the
# flagship's row view), 38 rows: one segment and two
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("kw", [5, 26])
def test_k_windows(kw, prec):
    hv = 1 if prec == "f32" else 2
    r = kw + 2 * hv
    expect = {kw: (r, 128 // kw + (128 % kw > 0), -(-38 * r // (1024 - 4 * r)))}
    assert expect[kw][2] == (1 if kw == 5 else 2)
    _case(prec, 40, 12, VEC[prec] * 128 - 4, [(kw, 3), (kw, WHOLE)], 4100 + kw, expect=expect)


# ---- 3. the march: chunks of 2 and 3 planes (general form only), 6, 7 and 10 (one group of four inner steps and what is left over), the whole
# box (fourteen planes: two groups and left-overs), and a j range that ends at nj (the inner form stops one step early)
MARCH_FORMS = [(0, 2), (0, 3), (0, 6), (0, 7), (0, 10), (0, WHOLE)]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("to_nj", [0, 1], ids=["box", "to_nj"])
def test_inner_and_general_steps(to_nj, prec):
    ni, nj, nk = 12, 16, 28
    idx = [2, ni - 1, 2, nj, 2, nk - 1] if to_nj else None
    _case(prec, ni, nj, nk, MARCH_FORMS, 5100 + to_nj, idx)


# ---- 4. the out-of-line division tail while the next stage's operands are held.  A wave leaves the gated tail of a stage when one of its 64
# numerators n = ss - b is huge, infinite or NaN -- in EVERY lane, also one whose result the update mask drops.
#   masked   huge values of b in the layer k = 1 (outside the inner box, so the update is dropped and nothing spreads), in planes j0 apart from
#            one another: the numerator of that cell alone is huge, in stage 1 at step j0, in stage 2 at step j0 + 1 (which works on plane
#            j0 with b(j0)), in stage 3 at step j0 + 2.  In each of these steps the wave takes the general tail in that ONE stage and the gated
#            tail in the other two; all other waves take the gated tail throughout.  The fields stay finite: residual sums to 1e-11.
#   all      the same and, nine planes and more away, cells inside the box with huge, infinite, NaN, -0, subnormal and tiny values in p and b: they
#            spread by one cell per sweep, so their waves take the general tail in stages 2 and 3 without stage 1 (the steps behind the
#            cell's plane), in stage 3 alone, and in all three.
def _planted(prec, shape, d, rng, inside):
    f = S.FMT[prec]
    R, U = f["R"], f["U"]
    hi1, hi2, lo = (100, 120, -120) if prec == "f32" else (772, 900, -1000)
    p, b = S.family("mixed", rng, shape, prec), S.family("mixed", rng, shape, prec)
    nj, ni, nk = shape
    # (array index = Fortran index + 1: k = 1 is index 2, the layer in front of the inner box)
    for j, i in ((4, 5), (8, ni - 5)):
        b[j, i, 2] = R(np.ldexp(float(d), hi1))
        b[j, i + 1, nk - 3] = R(-np.ldexp(1.0, hi2))  # (k = nk: the layer behind it)
    if inside:
        nan = np.array([0x7fc12345 if prec == "f32" else 0x7ff8000012345678], dtype=U).view(R)[0]
        sub = np.array([0x00012345], dtype=U).view(R)[0]
        vals = [R(np.ldexp(float(d), hi1)), R(-np.ldexp(1.0, hi2)), R(np.inf), R(-np.inf), nan, R(-0.0), sub, R(np.ldexp(1.0, lo))]
        n = 0
        for arr in (p, b):
            for j in (17, 20):
                for i in (4, ni - 5):
                    for k in (3, 9, nk // 2, nk - 6):
                        arr[j, i, k] = vals[n % len(vals)]
                        n += 1
    return p, b


@pytest.mark.parametrize("inside", [0, 1], ids=["masked", "all"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_general_tail_in_one_stage_of_a_step(prec, inside):
    from cubez_amd import CzHip
    ni, nj, nk = 12, 24, 60
    sz, idx = [ni, nj, nk], [2, ni - 1, 2, nj - 1, 2, nk - 1]
    h, ko = CzHip(prec), O.Kernels("oracle", prec)
    rng = np.random.default_rng(6100 + inside)
    cf = S.coef(ko.real, 1)
    p, b = _planted(prec, (nj + 4, ni + 4, nk + 4), cf[6], rng, inside)
    want, res = _three_oracle_sweeps(ko, p, b, sz, idx, cf)
    if inside:
        assert np.isnan(want).any() and np.isinf(want).any(), "the planted cells did not reach the result"
    else:
        assert np.isfinite(want).all() and np.isfinite(res).all()
    _check_forms(h, p, b, sz, idx, cf, want, res, [(0, 0), (5, 0), (0, 3), (0, WHOLE)], nans=bool(inside))
