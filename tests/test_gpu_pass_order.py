"""GPU tests (-m gpu) of the workgroup order and the chunk plan of the multi-stage passes (plan_pass / launch_pass, cz_h_launch.h): under
every order of czhip_set_pair_map (0 whole-segment bands, 1 row bands of every k window, 2 window-major) and chunk lengths from two planes
to all of them, the output equals the oracle's bit for bit and every sweep's residual equals the oracle's wide sum.  The output array starts
as a copy of the input, so an item no workgroup runs leaves stale values behind, and an item run twice counts its points twice in the
residual: both fail here."""
import numpy as np
import pytest

from oracle import cz_oracle as O

pytestmark = pytest.mark.gpu

ORDERS = [0, 1, 2]
# boxes whose rows are cut into k windows of 5 vectors: k extents that are no multiple of the vector width (nk + 4 = 201, 255), windows of
# unequal length (the last window of a row shorter), one chunk round (9 x 7 x 1100) and many (20 x 140 x 197 in chunks of 2 planes)
BOXES = [((9, 7, 1100), None), ((20, 140, 197), None), ((33, 20, 251), None)]
BOX_IDS = ["9x7x1100", "20x140x197", "33x20x251"]
# planes per chunk: the launcher's rule, 2, more than 128, and all planes (clamped to the box)
CHUNKS = [0, 2, 129, 100000]
KWIN = 5


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _problem(prec, box, seed):
    (ni, nj, nk), idx = box
    sz = [ni, nj, nk]
    idx = list(idx) if idx else [2, ni - 1, 2, nj - 1, 2, nk - 1]
    ko = O.Kernels("oracle", prec)
    R = ko.real
    rng = np.random.default_rng(seed + 11 * ni + 5 * nj + 3 * nk)
    shape = (nj + 4, ni + 4, nk + 4)
    cf = rng.uniform(0.5, 1.5, 7).astype(R)
    cf[6] = 6.2
    p, b = (rng.uniform(-1, 1, shape).astype(R) for _ in range(2))
    return sz, idx, ko, cf, p, b


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("box", BOXES, ids=BOX_IDS)
def test_three_sweep_pass_every_order_and_chunk(prec, box):
    from cubez_amd import CzHip
    sz, idx, ko, cf, p, b = _problem(prec, box, 1)
    a, w, r = p.copy(), np.zeros_like(p), []
    for _ in range(3):
        wide = np.zeros(1)
        ko.jacobi(a, sz, idx, cf, 0.9, b, w, wide=wide)
        r.append(wide[0])
    h = CzHip(prec)
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    try:
        for order in ORDERS:
            h.lib.czhip_set_pair_map(order)
            for tj in CHUNKS:
                assert h.lib.czhip_set_jac3(2, KWIN, tj) == 0
                dw = h.alloc(sz, p)
                ok, r1, r2, r3 = h.jacobi3(du, dw, db, sz, idx, cf, 0.9)
                assert ok, (order, tj)
                assert dw.get().tobytes() == a.tobytes(), (order, tj)
                for got, want in zip((r1, r2, r3), r):
                    assert _rel(got, want) < 1e-11, (order, tj, got, want)
                dw.free()
    finally:
        h.lib.czhip_set_pair_map(1)
        h.lib.czhip_set_jac3(1, 0, 0)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("box", BOXES, ids=BOX_IDS)
def test_two_iteration_red_black_pass_every_order_and_chunk(prec, box):
    from cubez_amd import CzHip
    sz, idx, ko, cf, p, b = _problem(prec, box, 2)
    a, r = p.copy(), []
    for _ in range(2):
        wide = np.zeros(1)
        for color in (0, 1):
            ko.psor2sma_core(a, sz, idx, cf, 0, color, 1.3, b, wide=wide)
        r.append(wide[0])
    h = CzHip(prec)
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    try:
        for order in ORDERS:
            h.lib.czhip_set_pair_map(order)
            for tj in CHUNKS:
                assert h.lib.czhip_set_rb4(2, KWIN, tj) == 0
                dw = h.alloc(sz, p)
                ok, r1, r2 = h.rbsor4(du, dw, db, sz, idx, cf, 0, 1.3)
                assert ok, (order, tj)
                assert dw.get().tobytes() == a.tobytes(), (order, tj)
                assert _rel(r1, r[0]) < 1e-11 and _rel(r2, r[1]) < 1e-11, (order, tj)
                dw.free()
    finally:
        h.lib.czhip_set_pair_map(1)
        h.lib.czhip_set_rb4(1, 0, 0)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("box", BOXES, ids=BOX_IDS)
def test_windowed_two_sweep_pass_every_order_and_chunk(prec, box):
    from cubez_amd import CzHip
    sz, idx, ko, cf, p, b = _problem(prec, box, 3)
    a, w, r = p.copy(), np.zeros_like(p), []
    for _ in range(2):
        wide = np.zeros(1)
        ko.jacobi(a, sz, idx, cf, 0.9, b, w, wide=wide)
        r.append(wide[0])
    h = CzHip(prec)
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    try:
        h.lib.czhip_set_pair_window(KWIN)
        h.lib.czhip_set_pair_preload(0)
        for order in ORDERS:
            h.lib.czhip_set_pair_map(order)
            for tb in (512, 1024):
                for tj in CHUNKS:
                    assert h.set_tuning2(tb, 2, tj, 1)
                    dw = h.alloc(sz, p)
                    ok, r1, r2 = h.jacobi2(du, dw, db, sz, idx, cf, 0.9)
                    assert ok, (order, tb, tj)
                    assert dw.get().tobytes() == a.tobytes(), (order, tb, tj)
                    assert _rel(r1, r[0]) < 1e-11 and _rel(r2, r[1]) < 1e-11, (order, tb, tj)
                    dw.free()
    finally:
        h.lib.czhip_set_pair_map(1)
        h.lib.czhip_set_pair_preload(1)
        h.lib.czhip_set_pair_window(-1)
        h.set_tuning2(-2, 2, 0, 1)


def test_pair_map_setting_round_trips():
    """czhip_set_pair_map returns the setting in force; the default is 1 (row bands)."""
    from cubez_amd import CzHip
    h = CzHip("f32")
    assert h.lib.czhip_set_pair_map(-1) == 1
    assert h.lib.czhip_set_pair_map(2) == 1
    assert h.lib.czhip_set_pair_map(1) == 2
