"""GPU tests (-m gpu) of how the three-sweep Jacobi pass (jac3_k) keeps a plane step's requests in flight across the step's barrier: the outer
rows of a u plane are requested two planes ahead by the waves that stage them and written to LDS after the first stage of the following step, the first
of them primed by the prologue; the inner steps come in groups of four whose right-hand-side registers rotate by name.  Every case is one
pass against three oracle sweeps (fields bit for bit, the input untouched, the three residual sums to 1e-11: the helper of
test_gpu_jac3_steps.py), at the smallest shapes at which that staging can go wrong:
    chunks of 2 .. 11 planes     no inner step, one to three left over in front of or behind a group of four, one and two groups; the first
                                 step's outer rows come from the prologue alone
    the array's end              a j range that ends at the array's last inner plane: the request of u(q+2) outer rows is clamped and limited
    segments and windows         two row segments (the outer rows are another workgroup's rows) and one; the rows below row 0 and behind the
                                 last row, clamped; first, middle and last k window
    outer row against the wave   R = 7 / 9 (inside one wave, TB - R inside the last wave), R = 64 (exactly one wave), R = 100 (two waves must
                                 request; TB - R = 924 inside wave 14)
in FP32 and FP64, with unit and with general coefficients.  The row length R, the number of k windows and the number of row segments per
window that a case is meant to run at are stated with it and checked against the launcher's rule (`_geometry`, restated from launch_deep and
plan_pass, cz_h_launch.h): window 0 in czhip_set_jac3 is that rule's own choice (26 / 36 vectors), not whole rows -- whole rows of Rfull
vectors are asked for with a window of Rfull."""
import numpy as np
import pytest

from oracle import cz_oracle as O
from test_gpu_jac3_steps import WHOLE, _check_forms, _coef, _three_oracle_sweeps

pytestmark = pytest.mark.gpu


def _geometry(prec, sz, idx, kwin):
    """(R, k windows, row segments per window) of the pass launch_deep plans for jac3_k on this box: TB = 1024 vectors per workgroup, four halo rows"""
    v, hv = (4, 1) if prec == "f32" else (2, 2)
    rfull = -(-(sz[2] + 4) // v)
    want = kwin if kwin > 0 else (26 if v == 4 else 36)
    r, nwin = rfull, 1
    if rfull > want + 2 * hv:
        nwin = -(-rfull // want)
        r = -(-rfull // nwin) + 2 * hv
    assert r <= 128, "the launcher declines rows of more than TB / 8 vectors"
    rows = idx[1] - idx[0] + 1
    return r, nwin, -(-rows * r // (1024 - 4 * r))


def _case(prec, unit, sz, idx, forms, seed, expect=None):
    from cubez_amd import CzHip
    ni, nj, nk = sz
    if expect is not None:  # the shape the case is about, for every form it runs
        for kw, _ in forms:
            assert _geometry(prec, sz, idx, kw) == expect, (prec, sz, kw, _geometry(prec, sz, idx, kw), expect)
    h, ko = CzHip(prec), O.Kernels("oracle", prec)
    R = ko.real
    rng = np.random.default_rng(seed)
    cf = _coef(R, unit, rng)
    p, b = (rng.uniform(-1, 1, (nj + 4, ni + 4, nk + 4)).astype(R) for _ in range(2))
    want, res = _three_oracle_sweeps(ko, p, b, sz, idx, cf)
    _check_forms(h, p, b, sz, idx, cf, want, res, forms)


def _box(sz, j1=None):
    ni, nj, nk = sz
    return [2, ni - 1, 2, nj - 1 if j1 is None else j1, 2, nk - 1]


# ---- 1. chunk lengths: 22 inner planes cut into chunks of 2 .. 11 (the last chunk of a box is shorter where the length does not divide 22:
# 22 = 3 * 6 + 4 = 2 * 8 + 6 = 2 * 9 + 4 ...), whole rows and windows of 5 vectors
@pytest.mark.parametrize("unit", [0, 1], ids=["coef", "unit"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_chunks_of_2_to_11_planes(prec, unit):
    sz = [12, 24, 28]
    _case(prec, unit, sz, _box(sz), [(0, tj) for tj in range(2, 12)] + [(5, tj) for tj in (2, 5, 7, 9)], 2000 + unit)


# ---- 2. the array's end: j = 2 .. nj, chunks that end there after no inner step, after a pair, after one and two groups of four
@pytest.mark.parametrize("unit", [0, 1], ids=["coef", "unit"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_requests_clamped_at_the_arrays_last_plane(prec, unit):
    sz = [12, 14, 28]
    _case(prec, unit, sz, _box(sz, j1=14), [(0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (0, WHOLE), (5, 6), (5, WHOLE)], 2100 + unit)


# ---- 3. segments and windows: rows of 60 elements are three (FP32) / six (FP64) windows of 5 vectors, R = 7 / 9, S = 996 / 988 own vectors per
# workgroup: the 148 rows of the box are 1 036 / 1 332 vectors = two segments, 10 rows one
@pytest.mark.parametrize("unit", [0, 1], ids=["coef", "unit"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("ni", [150, 12], ids=["two_segments", "one_segment"])
def test_outer_rows_of_first_middle_and_last_segment_and_window(ni, prec, unit):
    sz = [ni, 10, 56]
    expect = (7, 3, 2 if ni == 150 else 1) if prec == "f32" else (9, 6, 2 if ni == 150 else 1)
    _case(prec, unit, sz, _box(sz), [(5, 0), (5, 3)], 2200 + ni + unit, expect)
    _case(prec, unit, sz, _box(sz, j1=10), [(5, 0)], 2300 + ni + unit, expect)


# ---- 4. the outer row against the wave: whole rows (a window of Rfull vectors) of exactly 64 vectors, one segment, and of 100 in two
# segments (S = 624, 8 rows): the outer row spans waves 0 and 1 / 14 and 15, and is another workgroup's row
@pytest.mark.parametrize("unit", [0, 1], ids=["coef", "unit"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("wide", [0, 1], ids=["R64", "R100"])
def test_outer_row_of_one_wave_and_of_two(wide, prec, unit):
    v = 4 if prec == "f32" else 2
    nk = (64 * v if not wide else 400 if prec == "f32" else 200) - 4
    r = 100 if wide else 64
    sz = [10 if wide else 8, 8, nk]
    expect = (r, 1, 2 if wide else 1)
    _case(prec, unit, sz, _box(sz), [(r, 0), (r, 3)], 2400 + wide + unit, expect)
    _case(prec, unit, sz, _box(sz, j1=8), [(r, 0)], 2500 + wide + unit, expect)
