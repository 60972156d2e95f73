"""Zeros, subnormals, tiny and huge numerators in every stage of the passes that divide (-m gpu).  The families and what
they reach are tests/special_operands.py's, the conditions on them are checked on the oracle by tests/test_special_operands.py; here every
listed kernel form must be launched and give the oracle's sweeps bit for bit with its input untouched, and the residual sums must be 0.0 (sub,
tiny: the squares underflow in REAL), +inf (huge: they overflow; a NaN would mean a reduction that subtracts) or the oracle's to 1e-11 (mixed).

stencil_k (single sweeps: the plain n / d), jacobi2p_k (two Jacobi sweeps, unit and general coefficients, one red-black iteration), jac3_k
(three sweeps, FP32 with the medium and with the hoisted division, FP64) and rb4_k (two red-black iterations), on boxes with rows of 64 and
65 elements, k windows of 6 vectors as well as the launcher's rule; then the passes that build their divisor differently: pair_shell_k (the
shell slabs of a decomposed brick), the pass from a literal zero, the MAF pair and the multigrid level kernels (a divisor per point)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import special_operands as S  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
OMG_J, OMG_RB = 0.9, 1.3
BOX_IDS = ["x".join(map(str, g)) for g in S.BOXES]
PAIR_TUNINGS = [(-2, 2, 0), (512, 2, 5)]  # the library's choice; 512 threads, 2 vectors a thread, chunks of 5 planes
WINDOWS = [-1, 6]  # the launcher's rule; k windows of 6 vectors
FORMS3 = [(0, 0), (5, 0), (0, 3)]  # jac3_k: (vectors per k window, planes per chunk)
FORMS4 = [(0, 0), (5, 0), (0, 7)]  # rb4_k


def _case(family, prec, box):
    from cubez_amd import CzHip
    ni, nj, nk = box
    sz, idx = [ni, nj, nk], [2, ni - 1, 2, nj - 1, 2, nk - 1]
    p, b = S.fields(family, prec, (nj + 4, ni + 4, nk + 4))
    return CzHip(prec), O.Kernels("oracle", prec), sz, idx, p, b


class _Counted:
    """the launch inside the block was recorded once under `label` (the kernel the form belongs to, not another pass that gives the same bits),
    and the thread's settings in force are the forced ones: `want` against czhip_tuning_describe"""

    def __init__(self, h, label, what, **want):
        self.h, self.label, self.what, self.want = h, label, what, want

    def __enter__(self):
        t = self.h.tuning()
        assert all(t[k] == v for k, v in self.want.items()), (self.what, self.want, {k: t[k] for k in self.want})
        self.before = self.h.timing_read(self.label)[0]

    def __exit__(self, et, ev, tb):
        if et is None:
            n = self.h.timing_read(self.label)[0] - self.before
            assert n == 1, (self.what, f"{n} launches recorded under {self.label}")
        return False


@pytest.fixture(autouse=True)
def _timing():
    """launch counts per label on the calling thread, both libraries"""
    from cubez_amd import CzHip
    hs = [CzHip(q) for q in ("f32", "f64")]
    for h in hs:
        h.timing(True)
    yield
    for h in hs:
        h.timing(False)


def _same(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(f"u{got.itemsize}") != want.view(f"u{got.itemsize}"))
        print(f"{what}: {len(bad)} points differ, first (j, i, k) = {bad[:6].tolist()}, got {[got[tuple(q)] for q in bad[:3]]} want {[want[tuple(q)] for q in bad[:3]]}")
    assert got.tobytes() == want.tobytes(), what


def _residual(family, got, want, what):
    print(f"{what}: residual sum {got!r} oracle {want!r}")
    if family in ("sub", "tiny"):
        assert want == 0.0 and got == 0.0, (what, got)
    elif family == "huge":
        assert want == math.inf and got == math.inf, (what, got)
    else:
        assert abs(got - want) <= 1e-11 * abs(want), (what, got, want)


@pytest.mark.parametrize("box", S.BOXES, ids=BOX_IDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("family", S.FAMILIES)
def test_single_sweeps(family, prec, box):
    """stencil_k: jacobi and psor2sma_core (both colours, both offsets), unit and general coefficients"""
    h, ko, sz, idx, p, b = _case(family, prec, box)
    db = h.alloc(sz, b)
    for unit in (1, 0):
        cf = S.coef(ko.real, unit)
        want, res, _ = S.jacobi_sweeps(ko, p, b, sz, idx, cf, OMG_J, 1)
        dp, dw = h.alloc(sz, p), h.alloc(sz, np.zeros_like(p))
        r = h.jacobi(dp, sz, idx, cf, OMG_J, db, dw)
        _same(dp.get(), want, (family, prec, box, unit, "jacobi"))
        _residual(family, r, res[0], (family, prec, box, unit, "jacobi"))
        dp.free(), dw.free()
        for ofst in (0, 1):
            a, wide = p.copy(), np.zeros(1)
            dp, r = h.alloc(sz, p), 0.0
            for colour in (0, 1):
                ko.psor2sma_core(a, sz, idx, cf, ofst, colour, OMG_RB, b, wide=wide)
                r = h.psor2sma_core(dp, sz, idx, cf, ofst, colour, OMG_RB, db, res=r)
                _same(dp.get(), a, (family, prec, box, unit, "psor2sma_core", ofst, colour))
            _residual(family, r, float(wide[0]), (family, prec, box, unit, "psor2sma_core", ofst))
            dp.free()
    db.free()


@pytest.mark.parametrize("box", S.BOXES, ids=BOX_IDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("family", S.FAMILIES)
def test_two_sweeps_and_one_red_black_iteration(family, prec, box):
    """jacobi2p_k: jacobi2 with unit and general coefficients (the unit form and, with czhip_set_unit_coef(0), the general form on unit
    coefficients: the same bits) and rbsor2 with both offsets; the library's tuning and (512, 2, 5); k windows by the rule and of 6 vectors"""
    h, ko, sz, idx, p, b = _case(family, prec, box)
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    jac = {unit: S.jacobi_sweeps(ko, p, b, sz, idx, S.coef(ko.real, unit), OMG_J, 2) for unit in (1, 0)}
    rb = {(unit, ofst): S.colour_sweeps(ko, p, b, sz, idx, S.coef(ko.real, unit), OMG_RB, ofst, 1) for unit in (1, 0) for ofst in (0, 1)}
    try:
        for win in WINDOWS:
            h.lib.czhip_set_pair_window(win)
            for tb, mv, tj in PAIR_TUNINGS:
                assert h.set_tuning2(tb, mv, tj, 1)
                forced = dict(t2_kwin=win, use_t2=1, **(dict(t2_threads=tb, t2_mv=mv, t2_tj=tj) if tb > 0 else {}))
                for unit, forced_general in ((1, 0), (1, 1), (0, 0)):
                    cf = S.coef(ko.real, unit)
                    h.lib.czhip_set_unit_coef(0 if forced_general else 1)
                    what = (family, prec, box, win, (tb, mv, tj), unit, forced_general)
                    want, res, _ = jac[unit]
                    dw = h.alloc(sz, p)
                    with _Counted(h, "jacobi2", what, unit_coef=0 if forced_general else 1, **forced):
                        ok, r1, r2 = h.jacobi2(du, dw, db, sz, idx, cf, OMG_J)
                    assert ok, (what, "jacobi2: the launcher declined")
                    _same(dw.get(), want, what + ("jacobi2",))
                    _same(du.get(), p, what + ("jacobi2 input",))
                    _residual(family, r1, res[0], what + ("jacobi2", 1))
                    _residual(family, r2, res[1], what + ("jacobi2", 2))
                    dw.free()
                    for ofst in (0, 1):
                        want, res, _ = rb[unit, ofst]
                        dw = h.alloc(sz, p)
                        with _Counted(h, "rbsor2", what, **forced):
                            ok, r = h.rbsor2(du, dw, db, sz, idx, cf, ofst, OMG_RB)
                        assert ok, (what, ofst, "rbsor2: the launcher declined")
                        _same(dw.get(), want, what + ("rbsor2", ofst))
                        _same(du.get(), p, what + ("rbsor2 input",))
                        _residual(family, r, res[0], what + ("rbsor2", ofst))
                        dw.free()
    finally:
        h.lib.czhip_set_unit_coef(1)
        h.set_tuning2(-2, 2, 0, 1)
        h.lib.czhip_set_pair_window(-1)
        du.free(), db.free()


@pytest.mark.parametrize("box", S.BOXES, ids=BOX_IDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("family", S.FAMILIES)
def test_three_sweeps(family, prec, box):
    """jac3_k: forms (0, 0), (5, 0), (0, 3), unit and general coefficients; FP32 with the medium division and with the hoisted one"""
    h, ko, sz, idx, p, b = _case(family, prec, box)
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    try:
        for medium in ((1, 0) if prec == "f32" else (1,)):
            h.lib.czhip_set_jac3_medium(medium)
            for unit in (1, 0):
                cf = S.coef(ko.real, unit)
                want, res, _ = S.jacobi_sweeps(ko, p, b, sz, idx, cf, OMG_J, 3)
                for kw, tj in FORMS3:
                    what = (family, prec, box, medium, unit, (kw, tj), "jacobi3")
                    assert h.lib.czhip_set_jac3(2, kw, tj) == 0
                    dw = h.alloc(sz, p)
                    with _Counted(h, "jacobi3", what, jac3=2, jac3_kwin=kw, jac3_tj=tj, jac3_medium=medium):
                        ok, *rs = h.jacobi3(du, dw, db, sz, idx, cf, OMG_J)
                    assert ok, (what, "the launcher declined")
                    _same(dw.get(), want, what)
                    _same(du.get(), p, what + ("input",))
                    for s, (got_r, want_r) in enumerate(zip(rs, res), 1):
                        _residual(family, got_r, want_r, what + (s,))
                    dw.free()
    finally:
        h.lib.czhip_set_jac3_medium(1)
        h.lib.czhip_set_jac3(1, 0, 0)
        du.free(), db.free()


@pytest.mark.parametrize("box", S.BOXES, ids=BOX_IDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("family", S.FAMILIES)
def test_two_red_black_iterations(family, prec, box):
    """rb4_k: rbsor4 in the forms (0, 0), (5, 0), (0, 7), both offsets, unit and general coefficients"""
    h, ko, sz, idx, p, b = _case(family, prec, box)
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    try:
        for unit in (1, 0):
            cf = S.coef(ko.real, unit)
            for ofst in (0, 1):
                want, res, _ = S.colour_sweeps(ko, p, b, sz, idx, cf, OMG_RB, ofst, 2)
                for kw, tj in FORMS4:
                    what = (family, prec, box, unit, ofst, (kw, tj), "rbsor4")
                    assert h.lib.czhip_set_rb4(2, kw, tj) == 0
                    dw = h.alloc(sz, p)
                    with _Counted(h, "rbsor4", what, rb4=2, rb4_kwin=kw, rb4_tj=tj):
                        ok, r1, r2 = h.rbsor4(du, dw, db, sz, idx, cf, ofst, OMG_RB)
                    assert ok, (what, "the launcher declined")
                    _same(dw.get(), want, what)
                    _same(du.get(), p, what + ("input",))
                    _residual(family, r1, res[0], what + (1,))
                    _residual(family, r2, res[1], what + (2,))
                    dw.free()
    finally:
        h.lib.czhip_set_rb4(1, 0, 0)
        du.free(), db.free()


# ---- the passes with a FastDiv construction of their own: the shell slabs of a decomposed brick, the MAF pair (a divisor per point), the
# first pass of a preconditioner solve, the multigrid level kernels (a divisor per point from the level's weights)
SPLIT_PATTERN = [0, 1, 0, 0, 0, 1]  # neighbours on X+ and Z+: two faces, one of them along the rows


@pytest.mark.parametrize("rb", [-1, 0, 1], ids=["jacobi", "rb_ofst0", "rb_ofst1"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("family", S.FAMILIES)
def test_shell_slabs_and_interior(family, prec, rb):
    """pair_shell_k through czhip_pair_split_async: the first sweep (colour) one layer into the neighbours' ghost cells, the second on the
    brick's own box; the output box bit for bit the oracle's two sweeps, everything outside it untouched"""
    box = S.BOXES[0]
    h, ko, sz, _, p, b = _case(family, prec, box)
    n = [box[0], box[0], box[1], box[1], box[2], box[2]]
    nID = [(3 if v else -1) for v in SPLIT_PATTERN]
    idx = [(1 if v else 2) if f % 2 == 0 else (n[f] if v else n[f] - 1) for f, v in enumerate(SPLIT_PATTERN)]
    idx1 = [idx[f] + ((1 if f % 2 else -1) if v else 0) for f, v in enumerate(SPLIT_PATTERN)]
    w0 = S.fields("mixed", prec, p.shape, seed=11)[0]  # what must survive outside the output box
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    try:
        for unit in (1, 0):
            cf = S.coef(ko.real, unit)
            what = (family, prec, rb, unit, "pair_split")
            if rb < 0:
                want, res, _ = S.jacobi_sweeps(ko, p, b, sz, idx, cf, OMG_J, 2, idx_first=idx1)
            else:
                want, res, _ = S.colour_sweeps(ko, p, b, sz, idx, cf, OMG_RB, rb, 1, idx_first=idx1)
            dw = h.alloc(sz, w0)
            with _Counted(h, "pair_shell", what):
                ok, r1, r2 = h.pair_split(du, dw, db, sz, idx, idx1, nID, cf, OMG_J if rb < 0 else OMG_RB, rb_ofst=rb)
            assert ok, (what, "the launcher declined")
            ref = w0.copy()
            ref[S.inner(sz, idx)] = want[S.inner(sz, idx)]
            _same(dw.get(), ref, what)
            _same(du.get(), p, what + ("input",))
            if family != "mixed":  # (0.0 / +inf whichever box a sum is taken over; mixed: the sums of a brick count its own box, compared below)
                _residual(family, r1, res[0], what + (1,))
                if rb < 0:
                    _residual(family, r2, res[1], what + (2,))
            elif rb < 0:
                _residual(family, r2, res[1], what + (2,))
            dw.free()
    finally:
        du.free(), db.free()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("family", ["sub", "tiny"])
def test_maf_pair_on_a_stretched_grid(family, prec):
    """czhip_pair_maf_async: the divisor is made per point from the grid's spacings; two jacobi_maf sweeps and one red-black iteration of the
    oracle, both offsets"""
    from test_gpu_kernels import _coords
    box = S.BOXES[1]
    h, ko, sz, idx, p, b = _case(family, prec, box)
    rng = np.random.default_rng(77)
    xc, yc, zc = (_coords(rng, n, ko.real) for n in box)
    a1, w1, res = p.copy(), np.zeros_like(p), []
    for _ in range(2):
        wide = np.zeros(1)
        ko.jacobi_maf(a1, sz, idx, xc, yc, zc, OMG_J, b, w1, res=0.0, wide=wide)
        assert np.isfinite(a1).all()
        res.append(float(wide[0]))
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    try:
        for tb, mv, tj in PAIR_TUNINGS:
            assert h.set_tuning2(tb, mv, tj, 1)
            what = (family, prec, (tb, mv, tj), "pair_maf")
            dw = h.alloc(sz, p)
            ok, r1, r2 = h.pair_maf(du, dw, db, sz, idx, xc, yc, zc, OMG_J)
            assert ok, (what, "the launcher declined")
            _same(dw.get(), a1, what)
            _same(du.get(), p, what + ("input",))
            _residual(family, r1, res[0], what + (1,))
            _residual(family, r2, res[1], what + (2,))
            for ofst in (0, 1):
                a, wide = p.copy(), np.zeros(1)
                for colour in (0, 1):
                    ko.psor2sma_core_maf(a, sz, idx, xc, yc, zc, ofst, colour, OMG_RB, b, wide=wide)
                ok, r, _ = h.pair_maf(du, dw, db, sz, idx, xc, yc, zc, OMG_RB, rb_ofst=ofst)
                assert ok, (what, ofst, "the launcher declined")
                _same(dw.get(), a, what + ("rb", ofst))
                _residual(family, r, float(wide[0]), what + ("rb", ofst))
            dw.free()
    finally:
        h.set_tuning2(-2, 2, 0, 1)
        du.free(), db.free()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("family", ["sub", "tiny"])
def test_multigrid_level_kernels(family, prec):
    """mg_smooth (from zero and from u), mg_rb (either colour, from u and from zero) and the tails at every level of 9x7x12 against
    tests/mg_parity.py / tests/mgrb_parity.py (numpy keeps subnormals): the level's divisor is made per point from its weights"""
    import mg_parity as M
    import mgrb_parity as RB
    from test_gpu_mg import _level_array, _put
    omg = 0.8
    h = _case(family, prec, S.BOXES[0])[0]
    R = h.real
    idx0, _ = O.range_inner_index([9, 7, 12], [-1] * 6)
    n0 = M.n0_of(idx0)
    rng = np.random.default_rng(31)
    arrays, tails = [], 0
    try:
        for l, n in enumerate(M.level_dims(n0)):
            sz, idx = _level_array(n)
            shape = (n[1], n[0], n[2])
            u, b = S.family(family, rng, shape, prec), S.family(family, rng, shape, prec)
            ins = M.inner(sz, idx)
            du, db, dw = _put(h, sz, idx, u), _put(h, sz, idx, b), _put(h, sz, idx, None)
            arrays += [du, db, dw]
            for src, ref in ((None, M.smooth(None, b, l, n0, omg)), (du, M.smooth(u, b, l, n0, omg))):
                assert np.isfinite(ref).all()
                assert h.mg_smooth(src, dw, db, sz, idx, l, n0, omg), (l, "mg_smooth declined")
                _same(dw.get()[ins], ref.astype(R), (family, prec, l, "mg_smooth", "from u" if src else "from zero"))
            for c in ((0, 1) if l > 0 else ()):  # (mg_rb_k serves the levels >= 1; level 0 is rb4_k / jacobi2p_k above)
                dx = _put(h, sz, idx, u)
                arrays.append(dx)
                assert h.mg_rb(dx, db, sz, idx, l, n0, omg, c), (l, "mg_rb declined")
                _same(dx.get()[ins], RB.sweep(u, b, l, n0, omg, c), (family, prec, l, "mg_rb", c, "from u"))
                dx = _put(h, sz, idx, u)
                arrays.append(dx)
                assert h.mg_rb(dx, db, sz, idx, l, n0, omg, c, zero=1)
                first = RB.sweep(None, b, l, n0, omg, c)
                assert h.mg_rb(dx, db, sz, idx, l, n0, omg, 1 - c, zero=2)
                _same(dx.get()[ins], RB.sweep(first, b, l, n0, omg, 1 - c), (family, prec, l, "mg_rb", c, "from zero"))
            dx = _put(h, sz, idx, None)
            arrays.append(dx)
            if l > 0 and h.mg_tail(dx, db, sz, idx, l, n0, omg):
                tails += 1
                _same(dx.get()[ins], M.vcycle(b, l, n0, omg), (family, prec, l, "mg_tail"))
            dx = _put(h, sz, idx, u)
            arrays.append(dx)
            if l > 0 and h.mg_tail_rb(dx, db, sz, idx, l, n0, omg):
                tails += 1
                _same(dx.get()[ins], RB.vcycle(b, l, n0, R(omg)), (family, prec, l, "mg_tail_rb"))
        assert tails >= 2, "no tail was launched"
    finally:
        h.sync()
        for a in arrays:
            a.free()


@pytest.mark.parametrize("box", S.BOXES, ids=BOX_IDS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("family", S.FAMILIES)
def test_first_pass_from_a_literal_zero(family, prec, box):
    """czhip_jacobi2_from_zero_made_async: the start vector is not read, the right-hand side is read (op 0) or made from the operands of
    blas_triad (op 1) / blas_bicg_1 (op 2) and stored; two Jacobi sweeps with unit coefficients, one red-black iteration with general ones
    and both offsets.  Output field and stored right-hand side bit for bit the oracle's (its vector kernel, then its sweeps from a cleared
    field).  The first stage divides -b alone: the operands are special_operands.zero_pass_operands (huge: one cell in six)"""
    h, ko, sz, idx, p, _ = _case(family, prec, box)
    x, y, z = S.zero_pass_operands(family, prec, p.shape)
    zero = np.zeros_like(p)
    dx, dy, dz = h.alloc(sz, x), h.alloc(sz, y), h.alloc(sz, z)
    try:
        for op in (0, 1, 2):
            b = S.zero_pass_rhs(ko, op, x, y, z, sz, idx)
            for rb, unit in ((-1, 1), (0, 0), (1, 0)):
                cf = S.coef(ko.real, unit)
                what = (family, prec, box, op, rb, "pass_from_zero")
                if rb < 0:
                    want, _, _ = S.jacobi_sweeps(ko, zero, b, sz, idx, cf, OMG_J, 2)
                else:
                    want, _, _ = S.colour_sweeps(ko, zero, b, sz, idx, cf, OMG_RB, rb, 1)
                dw, dbo = h.alloc(sz, zero), h.alloc(sz, z)
                with _Counted(h, "jacobi2" if rb < 0 else "rbsor2", what):
                    ok = h.pass_from_zero(dw, dbo, sz, idx, cf, OMG_J if rb < 0 else OMG_RB, op=op, x=dx, y=dy, z=dz, a=S.ZERO_A[op], bb=S.ZERO_BB, rb_ofst=rb)
                assert ok, (what, "the launcher declined")
                _same(dw.get(), want, what)
                _same(dbo.get(), b, what + ("right-hand side",))
                for d, host in ((dx, x), (dy, y), (dz, z)):
                    _same(d.get(), host, what + ("operand",))
                dw.free(), dbo.free()
    finally:
        dx.free(), dy.free(), dz.free()
