"""Face coefficients inside the multigrid hierarchy on the GPU (-m gpu), through the public interface only, every result
against the numpy restatement of tests/coefmg_parity.py: one cycle (cz_precondition) byte for byte, unit coefficients against the constant
cycle of the same handle, PCG iteration by iteration against the exact-dot restatement, the count of the sharp bubble, the state of the flag,
the refusals (the coarse overflow among them), Refined."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coef_parity as K  # noqa: E402
import coefmg_measured as CM  # noqa: E402
import coefmg_parity as G  # noqa: E402
import mg_parity as M  # noqa: E402
import problem_parity as PP  # noqa: E402
import project_parity as J  # noqa: E402
import test_gpu_neumann as TN  # noqa: E402
from test_gpu_periodic import _handle  # noqa: E402
from test_gpu_problem import _real, _torch  # noqa: E402

pytestmark = pytest.mark.gpu
OMG = {"mg": 0.8, "mgrb": 1.2}

# (shape, precision, smoother, CZ_MG_TAIL, field, state): (5,5,5) one level, the eight sweeps only; (9,7,12) odd extents, lone children, three
# levels inside the tail; (33,47,61) row ends off the vector width, levels on both sides of the tail boundary; (40,40,1100) rows longer than a
# block; (3,40,40) and (40,3,40) one inner point in a direction; (4,9,12) a periodic direction that comes down to one point
CYCLES = [
    ((5, 5, 5), "f32", "mg", 1, "random", "dirichlet"),
    ((5, 5, 5), "f64", "mgrb", 1, "bubble1000", "closed"),
    ((9, 7, 12), "f32", "mgrb", 1, "random", "channel"),
    ((9, 7, 12), "f64", "mg", 0, "bubble1000", "inflow"),
    ((9, 7, 12), "f64", "mgrb", 0, "ones", "closed"),
    ((33, 47, 61), "f32", "mg", 1, "bubble1000", "channel"),
    ((33, 47, 61), "f64", "mgrb", 1, "random", "inflow"),
    ((33, 47, 61), "f32", "mgrb", 0, "bubble1000", "dirichlet"),
    ((33, 47, 61), "f64", "mg", 0, "ones", "closed"),
    ((40, 40, 1100), "f32", "mgrb", 1, "random", "closed"),
    ((40, 40, 1100), "f64", "mg", 1, "bubble1000", "dirichlet"),
    ((3, 40, 40), "f32", "mg", 1, "random", "inflow"),
    ((3, 40, 40), "f64", "mgrb", 0, "bubble1000", "dirichlet"),
    ((40, 3, 40), "f64", "mg", 1, "random", "channel"),
    ((40, 3, 40), "f32", "mgrb", 1, "bubble1000", "closed"),
    ((4, 9, 12), "f32", "mg", 0, "random", "channel"),
    ((4, 9, 12), "f64", "mgrb", 1, "random", "channel"),
]


def _cycle_id(c):
    return "_".join(["x".join(map(str, c[0]))] + [str(v) for v in c[1:]])


def _with_coef(cz, beta, on=True):
    cz.set_face_coef(*beta)
    cz.set_coef_mg(on)
    assert cz.info()["face_coef"] == 1 and cz.info()["coef_mg"] == (1 if on else 0)


@pytest.mark.parametrize("c", CYCLES, ids=[_cycle_id(c) for c in CYCLES])
def test_one_cycle_is_the_restatements(c, monkeypatch):
    """z = M_beta^-1 r through cz_precondition: the restatement's bytes, the same bytes from a second cycle, and with unit coefficients the
    bytes of the same handle's constant cycle"""
    gsz, prec, kind, tail, field, name = c
    state = K.STATES[name]
    assert J.fits(gsz, state)
    monkeypatch.setenv("CZ_MG_TAIL", str(tail))
    sz, idx, ins, r = TN._cycle_rhs(prec, gsz)
    beta = K.FIELDS[field](gsz, prec)
    ref = G.apply(kind, G.hierarchy(beta, gsz, state), r, sz, idx, OMG[kind])[ins]
    cz = _handle(prec, list(gsz) + ["pcg", 1, OMG[kind], kind], state)
    try:
        plain = cz.precondition(r)[ins]
        _with_coef(cz, beta)
        z = cz.precondition(r)[ins]
        assert cz.precondition(r)[ins].tobytes() == z.tobytes(), "the second cycle differs"
        cz.set_coef_mg(False)
        assert cz.info()["coef_mg"] == 0 and cz.precondition(r)[ins].tobytes() == plain.tobytes()
    finally:
        cz.close()
    assert np.isfinite(z).all() and z.any()
    assert z.tobytes() == ref.tobytes(), float(np.abs(z - ref).max())
    if field == "ones":
        assert z.tobytes() == plain.tobytes()
    else:
        assert z.tobytes() != plain.tobytes()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("kind", ["mg", "mgrb"])
@pytest.mark.parametrize("name", list(K.PCG_STATES))
def test_unit_coefficients_give_the_constant_cycle(name, kind, prec):
    """beta = 1: the coefficient cycle's bytes equal the same handle's cycle with the flag off, at a box with levels on both sides of the tail"""
    gsz, state = (33, 47, 61), K.STATES[name]
    sz, idx, ins, r = TN._cycle_rhs(prec, gsz)
    cz = _handle(prec, list(gsz) + ["pcg", 1, OMG[kind], kind], state)
    try:
        _with_coef(cz, K.ones(gsz, prec), on=False)
        off = cz.precondition(r)[ins]
        cz.set_coef_mg(True)
        assert cz.info()["coef_mg"] == 1
        on = cz.precondition(r)[ins]
    finally:
        cz.close()
    assert off.any() and on.tobytes() == off.tobytes()


# ---- PCG against the exact-dot restatement
@pytest.mark.parametrize("c", G.PCG_CASES, ids=[c["id"] for c in G.PCG_CASES])
def test_pcg_against_the_exact_dot_restatement(c):
    """K iterations: FP32 bit for bit (field and history), FP64 within 2 E + 8 ulp with the history within its envelope
    (tests/test_coefmg_oracle.py holds the premise of every case)"""
    gsz, prec, state = c["gsz"], c["prec"], K.STATES[c["state"]]
    b, p, beta = G.case_problem(c)
    cz = _handle(prec, list(gsz) + ["pcg", c["K"], c["coef"], c["pc"]], state)
    try:
        cz.set_eps(1e-30)
        cz.set_coef_mg(True)  # (before the coefficients: in force once they are set)
        assert cz.info()["coef_mg"] == 0
        cz.set_face_coef(*beta)
        cz.set_rhs(b)
        cz.set_field(p)
        itr = cz.solve()
        got, hist, info = cz.field(), cz.history(), cz.info()
    finally:
        cz.close()
    assert itr == c["K"] and info["face_coef"] == 1 and info["coef_mg"] == 1 and info["cg_fused"] == 0 and info["mg_cycles"] == c["K"]
    if prec == "f32":
        ref = G.case_run(c)
        assert got.tobytes() == ref.P.tobytes(), c["id"]
        assert hist == [v for _, v in ref.history], c["id"]
    else:
        ref, E, Eh = G.envelope_f64(gsz, c["pc"], c["coef"], state, c["K"], b, p, beta, eps=1e-30)
        ok, worst = PP.f64_close(got, ref.P, E)
        assert ok, (c["id"], worst)
        okh, worsth = PP.f64_close(hist, [v for _, v in ref.history], Eh)
        assert okh, (c["id"], worsth)


@pytest.mark.parametrize("pc,coef", K.COUNT_RUNS)
def test_bubble1000_counts_are_the_recorded_ones(pc, coef):
    """(33, 47, 61) FP64 to eps 1e-8: the restatement's recorded count with the flag on, the scaled column of coef_parity.COUNTS with it off"""
    g = K.COUNT_BOX
    b, p = PP.problem(g, "f64", 0)
    cz = _handle("f64", list(g) + ["pcg", 300, coef, pc], K.STATES["dirichlet"])
    got = {}
    try:
        cz.set_eps(K.COUNT_EPS)
        cz.set_face_coef(*K.FIELDS["bubble1000"](g, "f64"))
        for on in (True, False):
            cz.set_coef_mg(on)
            cz.set_rhs(b)
            cz.set_field(p)
            got[on] = cz.solve()
            assert cz.info()["coef_mg"] == int(on)
    finally:
        cz.close()
    print(pc, coef, got)
    assert got == {True: CM.COUNTS["bubble1000", pc], False: K.COUNTS["bubble1000", pc][1]}


# ---- the state of the flag
def _solved(cz, b, p):
    cz.set_eps(1e-30)
    cz.set_rhs(b)
    cz.set_field(p)
    return cz.solve(), cz.field().tobytes(), cz.history()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_flag_before_after_and_across_state_changes(prec):
    """the flag set before the coefficients, after them, and kept across set_periodic / set_neumann give the bytes of a handle that reached
    the same state in the plain order; cz_setup clears the flag; a twin that never saw the flag gives the bytes of one where it was turned
    on and off again"""
    gsz = (33, 47, 61)
    args = list(gsz) + ["pcg", 4, 1.2, "mgrb"]
    b, p = PP.problem(gsz, prec, 2)
    beta = K.bubble(gsz, prec, 1000)
    px = ((0, 0, 1, 0, 0, 0), (1, 0, 0), False)  # periodic X, Neumann Y-

    ref = _handle(prec, args, px)
    try:
        _with_coef(ref, beta)
        want = _solved(ref, b, p)
        ref.set_coef_mg(False)
        scaled = _solved(ref, b, p)
    finally:
        ref.close()
    assert want[0] == 4 and want[1] != scaled[1]

    cz = _handle(prec, args)
    try:
        cz.set_coef_mg(True)
        assert cz.info()["coef_mg"] == 0  # no coefficients yet
        cz.set_face_coef(*beta)
        assert cz.info()["coef_mg"] == 1
        cz.set_neumann(px[0])
        cz.set_periodic(px[1])
        assert cz.info()["coef_mg"] == 1 and cz.info()["periodic"] == 1
        assert _solved(cz, b, p) == want
        cz.set_face_coef(None)
        assert cz.info()["coef_mg"] == 0
        cz.set_face_coef(*beta)  # the flag is remembered
        assert cz.info()["coef_mg"] == 1 and _solved(cz, b, p) == want
        cz.set_coef_mg(False)
        assert cz.info()["coef_mg"] == 0 and _solved(cz, b, p) == scaled
        cz.set_coef_mg(True)
        assert cz.setup(args) == 1
        assert cz.info()["coef_mg"] == 0 and cz.info()["face_coef"] == 0
        cz.set_neumann(px[0])
        cz.set_periodic(px[1])
        cz.set_face_coef(*beta)
        assert cz.info()["coef_mg"] == 0 and _solved(cz, b, p) == scaled  # cz_setup cleared the flag
    finally:
        cz.close()


def test_idle_with_jacobi_and_none():
    """accepted and idle where the preconditioner has no hierarchy: the solve is that of a handle without the flag"""
    gsz, prec = (9, 7, 12), "f64"
    b, p = PP.problem(gsz, prec, 1)
    beta = K.random(gsz, prec)
    for pc in ("jacobi", "none"):
        out = []
        for flag in (False, True):
            cz = _handle(prec, list(gsz) + ["pcg", 5, 0.8, pc])
            try:
                cz.set_face_coef(*beta)
                if flag:
                    cz.set_coef_mg(True)
                assert cz.info()["coef_mg"] == 0
                out.append(_solved(cz, b, p))
            finally:
                cz.close()
        assert out[0] == out[1] and out[0][0] == 5, pc


# ---- the refusals
def test_refusals_and_the_coarse_overflow(capfd):
    from cubez_amd import CZ
    gsz, prec = (33, 47, 61), "f32"
    n = 0
    fresh = CZ(prec, quiet=True)
    try:
        assert fresh.lib.cz_set_coef_mg(fresh.h, 1) == 0  # before cz_setup
        n += 1
    finally:
        fresh.close()
    maf = _handle(prec, [9, 7, 12, "jacobi_maf", 50, 0.8])
    try:
        assert maf.lib.cz_set_coef_mg(maf.h, 1) == 0 and maf.info()["coef_mg"] == 0
        n += 1
    finally:
        maf.close()
    b, p = PP.problem(gsz, prec, 3)
    args = list(gsz) + ["pcg", 3, 1.2, "mgrb"]
    # faces of 1e37: every level-0 face and diagonal (6e37) is finite in FP32, level 1's weights (4e37) and diagonal too, level 2's diagonal
    # (six sums of sixteen) is not.  The start is zero and the right-hand side of size 1e15, so that the residuals, the answer (of size
    # 1e-22) and every dot of the solve (r.r about 1e35, r.z about 1e-2) stay in FP32's range and above the breakdown threshold
    huge = [np.full(gsz, 1e37, dtype=np.float32) for _ in range(3)]
    b, p = b * np.float32(1e15), np.zeros_like(p)
    with np.errstate(over="ignore"):
        H = G.hierarchy(huge, gsz, K.STATES["dirichlet"])
    assert np.isfinite(H[0].D).all() and G.count_bad(H[:2]) == 0 and G.count_bad(H) > 0
    twin = _handle(prec, args)
    try:
        twin.set_face_coef(*huge)
        want = _solved(twin, b, p)
    finally:
        twin.close()
    assert want[0] == 3 and np.isfinite(want[2]).all()
    cz = _handle(prec, args)
    try:
        cz.set_face_coef(*huge)
        with pytest.raises(RuntimeError):
            cz.set_coef_mg(True)
        n += 1
        assert cz.info()["coef_mg"] == 0 and cz.info()["face_coef"] == 1
        assert _solved(cz, b, p) == want  # the scaled path
        # the flag went off with the refusal: good coefficients do not bring the hierarchy back
        cz.set_face_coef(*K.random(gsz, prec))
        assert cz.info()["coef_mg"] == 0
        # the overflow met inside cz_set_face_coef: refused there, the coefficients stay
        cz.set_coef_mg(True)
        assert cz.info()["coef_mg"] == 1
        with pytest.raises(RuntimeError):
            cz.set_face_coef(*huge)
        assert cz.info()["coef_mg"] == 0 and cz.info()["face_coef"] == 1
        assert _solved(cz, b, p) == want
    finally:
        cz.close()
    err = capfd.readouterr().err
    assert err.count("cz_set_coef_mg: ") == n and err.count("cz_set_face_coef: a coarse weight") == 1, err
    for why in ("cz_setup first", "MAF", "a coarse weight of the coefficient hierarchy is not finite and positive", "the scaled preconditioner runs"):
        assert why in err, why


def test_a_decomposed_run_is_refused(capfd):
    gsz = (32, 36, 40)

    def work(q):
        cz = _handle("f32", list(gsz) + ["pcg", 10, 0.8, "mg", 2, 1, 1])
        try:
            return cz.lib.cz_set_coef_mg(cz.h, 1), cz.info()["coef_mg"]
        finally:
            cz.close()

    assert TN._ranks("f32", (2, 1, 1), work) == [(0, 0)] * 2
    assert capfd.readouterr().err.count("cz_set_coef_mg: a decomposed run") == 2


# ---- Refined
def test_refined_with_the_coefficient_hierarchy():
    """the problem of test_gpu_coef.py::test_refined_with_coefficients (smooth(4) at 64^3): the flag on both libraries (in force on the FP32
    one, which preconditions), the FP64 answer to 1e-10 (the residual of the FP64 handle itself)"""
    from cubez_amd.refine import Refined
    _torch()
    gsz = (64, 64, 64)
    beta = K.smooth(gsz, "f64", 4)
    b, p = PP.problem(gsz, "f64", 0)
    r = Refined(gsz)
    try:
        r.set_face_coef(*beta)
        r.set_coef_mg(True)
        # (the FP64 handle only forms residuals: its set-up solver has no hierarchy, the flag is accepted and idle there)
        assert r.lo.info()["coef_mg"] == 1 and r.hi.info()["coef_mg"] == 0 and r.hi.info()["face_coef"] == 1
        r.set_rhs(b)
        r.set_field(p)
        _, ss0 = r.hi.get_residual()
        steps = r.solve(tol=1e-10)
        hist = list(r.history)
        _, ss1 = r.hi.get_residual()
        inner_on = sum(h[2] for h in hist)
        r.set_coef_mg(False)
        assert r.hi.info()["coef_mg"] == 0 and r.lo.info()["coef_mg"] == 0
    finally:
        r.close()
    print("outer steps", steps, "inner iterations", inner_on, hist)
    assert steps > 0 and hist[-1][1] <= 1e-10 and np.sqrt(ss1) <= 1e-10 * np.sqrt(ss0), hist
