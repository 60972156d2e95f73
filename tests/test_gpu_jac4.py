"""GPU tests (-m gpu) of the four-sweep Jacobi pass (jac4_k, czhip_jacobi4_async; FP32 -- the FP64 library keeps jac3_k and answers 0): the
kernel against four oracle sweeps and four stencil_k sweeps, fields bit for bit, residuals to the double-summation tolerance of DESIGN 3;
the driver's quads against the sequential loop of the oracle.  Everything at jac4 = 2 (small boxes)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import special_operands as S  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
OMG = 0.9
LV = 1024  # vectors a workgroup holds; its own are S = LV - 6 R

# (box, idx, forms, expected geometry of the first form).  A form is (vectors per k window, planes per chunk), 0 = the launcher's rule.
# Whole rows of 31, 32, 33, 63 and 64 vectors (nk + 4 = 4 R): wave boundaries (64 vectors) fall differently on the stage sets [s R, LV - s R).
# A whole row of 100 vectors would leave a workgroup 424 own vectors of 1024 -- the launcher refuses rows beyond 85 (half of the vectors
# must be owned) -- so that box is asserted to be refused whole and runs in windows.
WHOLE = lambda r: (r, 0)  # a window as long as the row: whole rows
CASES = [
    ((20, 9, 120), None, [WHOLE(31), (5, 2)], dict(R=31, S=LV - 6 * 31, nwin=1, nsegw=1)),            # one row segment (18 rows)
    ((40, 11, 124), None, [WHOLE(32), (0, 3)], dict(R=32, S=LV - 6 * 32, nwin=1, nsegw=2)),           # a short last segment: 38 rows = 832 + 384 vectors
    ((20, 9, 128), None, [WHOLE(33), (0, 1)], dict(R=33, S=LV - 6 * 33, nwin=1, nsegw=1)),
    ((14, 23, 248), None, [WHOLE(63), (26, 10), (26, 5)], dict(R=63, S=LV - 6 * 63, nwin=1, nsegw=2)),
    ((14, 23, 252), None, [WHOLE(64), (5, 7), (26, 0)], dict(R=64, S=LV - 6 * 64, nwin=1, nsegw=2)),
    ((9, 8, 396), None, [(0, 0), (26, 2), (5, 3)], dict(R=27, nwin=4, KT=25)),                        # rows of 100 vectors: windows
    ((14, 12, 61), None, [(0, 0), (5, 2), (0, 5)], dict(R=17, nwin=1)),                               # nkp % V != 0: the partial vector
    ((13, 10, 123), None, [(0, 0), (26, 3)], dict(R=18, nwin=2, KT=16)),                              # ... in the last of two windows
    ((24, 20, 28), (1, 24, 1, 20, 1, 28), [(0, 0), (5, 10)], dict(R=8, nwin=1)),                      # the box up to the array's first / last inner layers
    ((24, 20, 60), (3, 20, 4, 15, 5, 50), [(0, 0), (5, 7)], dict(R=16, nwin=1)),                      # a box inside: its last plane is not the array's
]
IDS = ["x".join(map(str, c[0])) + ("" if c[1] is None else "_idx") for c in CASES]


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _fields(box, idx, unit, R):
    ni, nj, nk = box
    sz = [ni, nj, nk]
    idx = list(idx) if idx else [2, ni - 1, 2, nj - 1, 2, nk - 1]
    rng = np.random.default_rng(5 * ni + 7 * nj + 3 * nk + unit)
    shape = (nj + 4, ni + 4, nk + 4)
    p, b = (rng.uniform(-1, 1, shape).astype(R) for _ in range(2))
    return sz, idx, S.coef(R, unit), p, b


@pytest.mark.parametrize("unit", [0, 1], ids=["coef", "unit"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_four_sweeps_per_pass_equal_four_sweeps(case, unit):
    """czhip_jacobi4_async == four oracle sweeps == four stencil_k sweeps, bit for bit, with the residuals of all four sweeps to 1e-11 of the
    oracle's double accumulation; the planned geometry is the one the case is about; every division form the context offers; the input is
    never modified."""
    from cubez_amd import CzHip
    box, idx, forms, geom = case
    h, ko = CzHip("f32"), O.Kernels("oracle", "f32")
    sz, idx, cf, p, b = _fields(box, idx, unit, ko.real)
    want, res, _ = S.jacobi_sweeps(ko, p, b, sz, idx, cf, OMG, 4)
    du, db, ds, dk = h.alloc(sz, p), h.alloc(sz, b), h.alloc(sz, p), h.alloc(sz, p)
    for _ in range(4):
        h.jacobi(ds, sz, idx, cf, OMG, db, dk)  # stencil_k, in place
    assert ds.get().tobytes() == want.tobytes()
    h.timing(True)
    try:
        assert h.lib.czhip_set_jac3(2, -1, -1) == 0
        for n, (kw, tj) in enumerate(forms):
            assert h.lib.czhip_set_jac4(2, kw, tj) == 0
            dw = h.alloc(sz, p)
            plan = h.jac4_plan(du, dw, db, sz, idx, cf, OMG)
            assert plan is not None, (kw, tj)
            if n == 0:
                assert {k: plan[k] for k in geom} == geom, plan
            if tj:
                assert plan["TJ"] == min(tj, idx[3] - idx[2] + 1), plan
            assert plan["S"] == LV - 6 * plan["R"] and 2 * plan["S"] >= LV and plan["lds"] <= 160 * 1024, plan
            # medium and hoisted division, gated and not (the gate and the medium form act where the divisor passed on this context)
            for medium, gate in ((1, 1), (0, 1), (1, 0), (0, 0)) if n == 0 else ((1, 1),):
                h.lib.czhip_set_jac3_medium(medium), h.lib.czhip_set_jac3_gate(gate)
                before = h.timing_read("jacobi4")[0]
                ok, *rs = h.jacobi4(du, dw, db, sz, idx, cf, OMG)
                assert ok and h.timing_read("jacobi4")[0] == before + 1, (kw, tj, medium, gate)
                assert dw.get().tobytes() == want.tobytes(), (kw, tj, medium, gate)
                assert du.get().tobytes() == p.tobytes()
                for s, (got, ref) in enumerate(zip(rs, res), 1):
                    print(f"{box} {(kw, tj)} div {(medium, gate)} sweep {s}: residual {got!r} oracle {ref!r} rel {_rel(got, ref):.2e}")
                    assert _rel(got, ref) < 1e-11, (kw, tj, s, got, ref)
                dw.put(p)
            dw.free()
    finally:
        h.lib.czhip_set_jac3_medium(1), h.lib.czhip_set_jac3_gate(1)
        h.lib.czhip_set_jac4(1, 0, 0), h.lib.czhip_set_jac3(1, 0, 0)
        h.timing(False)
        for a in (du, db, ds, dk):
            a.free()


def test_rows_of_100_vectors_are_refused_whole_and_fp64_keeps_three_sweeps():
    from cubez_amd import CzHip
    h = CzHip("f32")
    sz, idx, cf, p, b = _fields((9, 8, 396), None, 1, np.float32)
    du, db, dw = h.alloc(sz, p), h.alloc(sz, b), h.alloc(sz, p)
    try:
        h.lib.czhip_set_jac3(2, -1, -1)
        h.lib.czhip_set_jac4(2, 100, 0)
        assert h.jac4_plan(du, dw, db, sz, idx, cf, OMG) is None
        h.lib.czhip_set_jac4(2, 83, 0)  # the longest row a workgroup takes: 83 + 2 halo vectors
        plan = h.jac4_plan(du, dw, db, sz, idx, cf, OMG)
        assert plan is not None and plan["nwin"] == 2 and plan["R"] == 52, plan
        h.lib.czhip_set_jac3(0, -1, -1)  # jac4 is off whenever jac3 is off
        assert h.jac4_plan(du, dw, db, sz, idx, cf, OMG) is None
    finally:
        h.lib.czhip_set_jac4(1, 0, 0), h.lib.czhip_set_jac3(1, 0, 0)
        for a in (du, db, dw):
            a.free()
    h = CzHip("f64")
    sz, idx, cf, p, b = _fields((20, 9, 120), None, 1, np.float64)
    du, db, dw = h.alloc(sz, p), h.alloc(sz, b), h.alloc(sz, p)
    try:
        h.lib.czhip_set_jac3(2, -1, -1), h.lib.czhip_set_jac4(2, 0, 0)
        assert h.jacobi4(du, dw, db, sz, idx, cf, OMG, probe=1)[0] is False
        assert h.jacobi3(du, dw, db, sz, idx, cf, OMG, probe=1)[0] is True
    finally:
        h.lib.czhip_set_jac4(1, 0, 0), h.lib.czhip_set_jac3(1, 0, 0)
        for a in (du, db, dw):
            a.free()


@pytest.mark.parametrize("box", S.BOXES, ids=["x".join(map(str, g)) for g in S.BOXES])
@pytest.mark.parametrize("family", ["sub", "tiny", "huge"])
def test_special_operands_through_four_sweeps(family, box):
    """zeros and subnormals, tiny and huge numerators in all four stages: the oracle's bits; the residual sums are 0.0 (the squares underflow),
    +inf (they overflow) -- never a NaN"""
    from cubez_amd import CzHip
    ni, nj, nk = box
    sz, idx = [ni, nj, nk], [2, ni - 1, 2, nj - 1, 2, nk - 1]
    p, b = S.fields(family, "f32", (nj + 4, ni + 4, nk + 4))
    h, ko = CzHip("f32"), O.Kernels("oracle", "f32")
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    try:
        h.lib.czhip_set_jac3(2, -1, -1)
        for medium in (1, 0):
            h.lib.czhip_set_jac3_medium(medium)
            for unit in (1, 0):
                cf = S.coef(ko.real, unit)
                want, res, _ = S.jacobi_sweeps(ko, p, b, sz, idx, cf, OMG, 4)
                for kw, tj in [(0, 0), (5, 0), (0, 3)]:
                    h.lib.czhip_set_jac4(2, kw, tj)
                    dw = h.alloc(sz, p)
                    ok, *rs = h.jacobi4(du, dw, db, sz, idx, cf, OMG)
                    assert ok, (family, box, medium, unit, kw, tj)
                    assert dw.get().tobytes() == want.tobytes(), (family, box, medium, unit, kw, tj)
                    assert du.get().tobytes() == p.tobytes()
                    for got, ref in zip(rs, res):
                        assert not np.isnan(got) and (got == ref or _rel(got, ref) < 1e-11), (family, got, ref)
                    dw.free()
    finally:
        h.lib.czhip_set_jac3_medium(1)
        h.lib.czhip_set_jac4(1, 0, 0), h.lib.czhip_set_jac3(1, 0, 0)
        du.free(), db.free()


# ---- the inner form of the plane step.  A chunk reaches it with 13 planes or more (a group of ten steps from the first even step >= ja + 3
# must end by step jb, or by jb - 1 where jb is the array's last inner plane); every case above runs chunks of ten planes or fewer, so
# the general form only.  Here: chunks of 14, 17, 24, 27 planes and the whole range -- one, two and three groups of ten with left-over
# steps of the general form; chunks of 17 planes start at planes of both parities in one launch, so the fill takes six steps in one
# workgroup and seven (with the move of the pending requests) in the next; two j ranges, one of which ends at the array's last inner
# plane (the arm `jlast - 3` of the inner form's last step) and which start at planes of different parity.
INNER_BOX = (10, 36, 60)
INNER_IDX = [(2, 9, 1, 36, 2, 59), (2, 9, 2, 35, 2, 59)]  # 36 planes up to the array's last inner plane; 34 planes inside
INNER_FORMS = [(0, 17), (0, 14), (0, 24), (0, 27), (0, 36), (5, 17)]
DIVISIONS = ((1, 1), (0, 1), (1, 0), (0, 0))  # (medium, gate)


def _inner_run(h, sz, idx, cf, p, b, want, res, forms, divisions, what, exact_res=False):
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    h.timing(True)
    try:
        h.lib.czhip_set_jac3(2, -1, -1)
        for kw, tj in forms:
            h.lib.czhip_set_jac4(2, kw, tj)
            dw = h.alloc(sz, p)
            plan = h.jac4_plan(du, dw, db, sz, idx, cf, OMG)
            nplanes = idx[3] - idx[2] + 1
            assert plan is not None and plan["TJ"] == min(tj, nplanes) >= 14 and plan["nchunk"] == -(-nplanes // plan["TJ"]), (what, kw, tj, plan)
            for medium, gate in divisions:
                h.lib.czhip_set_jac3_medium(medium), h.lib.czhip_set_jac3_gate(gate)
                before = h.timing_read("jacobi4")[0]
                ok, *rs = h.jacobi4(du, dw, db, sz, idx, cf, OMG)
                assert ok and h.timing_read("jacobi4")[0] == before + 1, (what, kw, tj, medium, gate)
                assert dw.get().tobytes() == want.tobytes(), (what, kw, tj, medium, gate)
                assert du.get().tobytes() == p.tobytes()
                for s, (got, ref) in enumerate(zip(rs, res), 1):
                    assert not np.isnan(got) and (got == ref or _rel(got, ref) < 1e-11), (what, kw, tj, s, got, ref)
                dw.put(p)
            dw.free()
    finally:
        h.lib.czhip_set_jac3_medium(1), h.lib.czhip_set_jac3_gate(1)
        h.lib.czhip_set_jac4(1, 0, 0), h.lib.czhip_set_jac3(1, 0, 0)
        h.timing(False)
        du.free(), db.free()


@pytest.mark.parametrize("unit", [0, 1], ids=["coef", "unit"])
@pytest.mark.parametrize("idx", INNER_IDX, ids=["to_last_plane", "inside"])
def test_inner_steps_equal_four_sweeps(idx, unit):
    """chunks long enough for the inner form, both fills, one to three groups of ten, every division form, unit and general coefficients:
    four oracle sweeps bit for bit, four residuals to 1e-11"""
    from cubez_amd import CzHip
    h, ko = CzHip("f32"), O.Kernels("oracle", "f32")
    sz, idx, cf, p, b = _fields(INNER_BOX, idx, unit, ko.real)
    want, res, _ = S.jacobi_sweeps(ko, p, b, sz, idx, cf, OMG, 4)
    _inner_run(h, sz, idx, cf, p, b, want, res, INNER_FORMS, DIVISIONS, ("inner", tuple(idx), unit))


@pytest.mark.parametrize("family", ["sub", "tiny", "huge"])
def test_special_operands_through_inner_steps(family):
    """zeros and subnormals, tiny and huge numerators through the inner form of all four stages (chunks of 17 planes and the whole range,
    medium and hoisted division, gated and not, unit and general coefficients)"""
    from cubez_amd import CzHip
    ni, nj, nk = INNER_BOX
    h, ko = CzHip("f32"), O.Kernels("oracle", "f32")
    sz, idx = [ni, nj, nk], list(INNER_IDX[0])
    p, b = S.fields(family, "f32", (nj + 4, ni + 4, nk + 4))
    for unit in (1, 0):
        cf = S.coef(ko.real, unit)
        want, res, _ = S.jacobi_sweeps(ko, p, b, sz, idx, cf, OMG, 4)
        _inner_run(h, sz, idx, cf, p, b, want, res, [(0, 17), (0, 36)], DIVISIONS, (family, unit))


# ---- the driver
def _solve(gsz, itmax, coef, jac3, jac4, eps=None, t2=1):
    from cubez_amd import CZ
    cz = CZ("f32", quiet=True)
    cz.lib.czhip_set_jac3(jac3, -1, -1)
    cz.lib.czhip_set_jac4(jac4, -1, -1)
    cz.lib.czhip_set_tuning2(0, 0, -1, t2)
    try:
        assert cz.setup(list(gsz) + ["jacobi", itmax, coef]) == 1
        if eps is not None:
            cz.set_eps(eps)
        itr = cz.solve()
        return dict(itr=itr, res=cz.res, hist=list(cz.history()), P=cz.field().tobytes(), info=cz.info())
    finally:
        cz.lib.czhip_set_jac4(1, -1, -1)
        cz.lib.czhip_set_jac3(1, -1, -1)
        cz.lib.czhip_set_tuning2(0, 0, -1, 1)
        cz.close()


GSZ = (40, 36, 44)
_oracle = {}


def _oracle_run(itmax):
    """the sequential loop, once per length"""
    if itmax not in _oracle:
        _oracle[itmax] = O.run(GSZ, "jacobi", itmax, 0.8, None, kind="oracle", prec="f32", wide=True)
    return _oracle[itmax]


@pytest.mark.parametrize("itmax", [4, 5, 6, 7, 9, 11])
def test_fixed_iteration_counts_under_quads(itmax):
    """quads while four sweeps remain, then the triple, the pair or the single sweep"""
    g = _solve(GSZ, itmax, 0.8, 2, 2)
    o = _oracle_run(itmax)
    assert g["itr"] == o.itr == itmax + 1
    rest = itmax % 4
    assert g["info"]["jac4_passes"] == itmax // 4 and g["info"]["jac3_passes"] == (1 if rest == 3 else 0), g["info"]
    assert g["P"] == o.P.tobytes()
    assert np.allclose(g["hist"], [r for _, r in o.history], rtol=1e-11, atol=0)


@pytest.mark.parametrize("sweep", [1, 2, 3, 4])
def test_convergence_on_each_sweep_of_a_quad(sweep):
    """eps between two residuals of the oracle's history, so that the solve converges at iteration 8 + sweep -- sweep 1 .. 4 of the third quad.
    Iter, history and field equal the sequential loop; a converged sweep that is not the quad's last is re-run from the quad's input as
    one sweep, one pair or one three-sweep pass."""
    hist = [r for _, r in _oracle_run(16).history]  # hist[n - 1] = residual of iteration n
    n = 8 + sweep
    assert all(hist[i] > hist[i + 1] for i in range(n)), "the residual falls monotonically here"
    eps = float(np.sqrt(hist[n - 2] * hist[n - 1]))
    g = _solve(GSZ, 100, 0.8, 2, 2, eps=eps)
    o = _oracle_run(n)  # n sweeps of the sequential loop
    assert g["itr"] == n, (g["itr"], n)
    assert g["info"]["jac4_passes"] >= 3 and g["info"]["exact_reruns"] == (1 if sweep < 4 else 0), g["info"]
    assert g["P"] == o.P.tobytes()
    assert np.allclose(g["hist"][:n], hist[:n], rtol=1e-11, atol=0)


def test_switches_and_preconditioner_solves():
    """jac3 = 0 gives no four-sweep pass; jac4 at its default leaves small boxes to the triples; a preconditioner solve -- the only solve
    that starts from a literal zero and keeps a first pass of its own -- takes no four-sweep pass"""
    from cubez_amd import CZ
    o = _oracle_run(11)
    g = _solve(GSZ, 11, 0.8, 2, 2)
    assert g["P"] == o.P.tobytes()
    off = _solve(GSZ, 11, 0.8, 0, 2)
    assert off["info"]["jac4_passes"] == 0 and off["info"]["jac3_passes"] == 0 and off["P"] == o.P.tobytes(), off["info"]
    dflt = _solve(GSZ, 11, 0.8, 2, 1)
    assert dflt["info"]["jac4_passes"] == 0 and dflt["info"]["jac3_passes"] == 11 // 3 and dflt["P"] == o.P.tobytes(), dflt["info"]
    # a preconditioner solve starts from zero: pbicgstab with jacobi takes no four-sweep pass (quads only outside a preconditioner)
    cz = CZ("f32", quiet=True)
    cz.lib.czhip_set_jac3(2, -1, -1), cz.lib.czhip_set_jac4(2, -1, -1)
    try:
        assert cz.setup(list(GSZ) + ["pbicgstab", 3, 0.8, "jacobi"]) == 1
        cz.solve()
        assert cz.info()["jac4_passes"] == 0
    finally:
        cz.lib.czhip_set_jac4(1, -1, -1), cz.lib.czhip_set_jac3(1, -1, -1)
        cz.close()


def test_jacobi_512_quads_by_default_in_solves_of_eight_sweeps_or_more():
    """`cz 512 512 512 jacobi 9` (the headline workload, every switch at its default) takes two quads and a single sweep: == the oracle, bit for
    bit, history to 1e-11.  (Shorter solves keep their triples: tests/test_gpu_jac3.py.)"""
    N, nit = 512, 9
    g = _solve((N, N, N), nit, 0.8, 1, 1)
    assert g["info"]["jac4_passes"] == 2 and g["info"]["jac3_passes"] == 0 and g["info"]["pass_kind"] == 1, g["info"]
    o = O.run((N, N, N), "jacobi", nit, 0.8, kind="oracle", prec="f32", wide=True)
    assert g["itr"] == o.itr == nit + 1
    assert g["P"] == o.P.tobytes()
    assert np.allclose(g["hist"], [r for _, r in o.history], rtol=1e-11, atol=0)
