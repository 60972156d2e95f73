"""The zebra line smoother along Z on the GPU (-m gpu), through the public interface only, every result against the numpy
restatement of tests/lines_parity.py: one cycle (cz_precondition) byte for byte, the flag off again against a twin that never had it, PCG
iteration by iteration against the exact-dot restatement, the recorded counts of the stretched fields, the state of the flag, the refusals,
Refined."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coef_parity as K  # noqa: E402
import coefmg_parity as G  # noqa: E402
import lines_measured as LM  # noqa: E402
import lines_parity as LP  # noqa: E402
import problem_parity as PP  # noqa: E402
import project_parity as J  # noqa: E402
import test_gpu_neumann as TN  # noqa: E402
from test_gpu_periodic import _handle  # noqa: E402
from test_gpu_problem import _torch  # noqa: E402

pytestmark = pytest.mark.gpu
SIX = ("dirichlet", "inflow", "closed", "channel", "triple", "px")


def _chunk(prec):
    """C of the line kernel in this precision (no GPU is touched)"""
    from cubez_amd import lib
    so = ctypes.CDLL(lib.lib_path(prec))
    so.czhip_mg_line_chunk.restype = ctypes.c_int
    c = so.czhip_mg_line_chunk()
    assert 2 <= c <= 1024
    return c


# the boxes: (5,5,5) one level; (9,7,12) odd extents; (33,47,61) row ends off the vector width, rows of one colour on several workgroups;
# (5,5,40) comes down to levels of one row, which keep the point sweeps; (40,40,3) one-cell lines; (3,40,40) and (40,3,40) one inner point in
# a direction; (4,9,12) a periodic direction down to one point; lines of C - 1, C, C + 1 and 2 C + 1 cells around the kernel's chunk C;
# (40,40,1100) many chunks
FIXED = [(5, 5, 5), (9, 7, 12), (33, 47, 61), (5, 5, 40), (40, 40, 3), (3, 40, 40), (40, 3, 40), (4, 9, 12)]
AROUND = [("C+1", lambda c: c + 1), ("C+2", lambda c: c + 2), ("C+3", lambda c: c + 3), ("2C+3", lambda c: 2 * c + 3)]


def _cycles():
    out, i = [], 0
    boxes = [("x".join(map(str, g)), (lambda c, g=g: g)) for g in FIXED] + [(f"7x6x{n}", (lambda c, f=f: (7, 6, f(c)))) for n, f in AROUND]
    for label, box in boxes:
        for name in SIX:
            prec, field = ("f32", "f64")[i % 2], ("random", "stretch30")[(i // 2) % 2]
            g = box(8)  # (whether the state fits does not depend on C)
            i += 1
            if J.fits(g, K.STATES[name]):
                out.append(pytest.param(box, prec, name, field, id=f"{label}_{prec}_{name}_{field}"))
    for prec, name, field in (("f32", "channel", "stretch30"), ("f64", "inflow", "random"), ("f32", "closed", "random"), ("f64", "dirichlet", "stretch30")):
        out.append(pytest.param(lambda c: (40, 40, 1100), prec, name, field, id=f"40x40x1100_{prec}_{name}_{field}"))
    return out


def _with_lines(cz, beta):
    cz.set_face_coef(*beta)
    cz.set_coef_mg(True)
    cz.set_mg_lines(True)
    assert cz.info()["coef_mg"] == 1 and cz.info()["mg_lines"] == 1


@pytest.mark.parametrize("box,prec,name,field", _cycles())
def test_one_cycle_is_the_restatements(box, prec, name, field):
    """z = M^-1 r of the line cycle through cz_precondition: the restatement's bytes, the same bytes from a second cycle, and other bytes
    than the point cycle's"""
    gsz, state = box(_chunk(prec)), K.STATES[name]
    sz, idx, ins, r = TN._cycle_rhs(prec, gsz)
    beta = LP.FIELDS[field](gsz, prec)
    ref = LP.apply(G.hierarchy(beta, gsz, state), r, sz, idx, 1.0)[ins]
    cz = _handle(prec, list(gsz) + ["pcg", 1, 1.0, "mgrb"], state)
    try:
        cz.set_face_coef(*beta)
        cz.set_coef_mg(True)
        points = cz.precondition(r)[ins]
        cz.set_mg_lines(True)
        assert cz.info()["mg_lines"] == 1
        z = cz.precondition(r)[ins]
        assert cz.precondition(r)[ins].tobytes() == z.tobytes(), "the second cycle differs"
    finally:
        cz.close()
    assert np.isfinite(z).all() and z.any()
    assert z.tobytes() == ref.tobytes(), float(np.abs(z - ref).max())
    if gsz[2] > 3:  # (a one-cell line is the point update of the same colour)
        assert z.tobytes() != points.tobytes()


def _solved(cz, b, p):
    cz.set_eps(1e-30)
    cz.set_rhs(b)
    cz.set_field(p)
    return cz.solve(), cz.field().tobytes(), cz.history()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["dirichlet", "channel"])
def test_off_again_gives_the_bytes_of_a_twin_that_never_had_it(name, prec):
    """(33, 47, 61): the cycle and four iterations of a handle whose flag went on and off again against a twin that never saw it, under the
    coefficient hierarchy and without it"""
    gsz, state = (33, 47, 61), K.STATES[name]
    args = list(gsz) + ["pcg", 4, 1.0, "mgrb"]
    sz, idx, ins, r = TN._cycle_rhs(prec, gsz)
    b, p = PP.problem(gsz, prec, 2)
    beta = LP.stretch(gsz, prec, 30)
    twin = _handle(prec, args, state)
    try:
        twin.set_face_coef(*beta)
        scaled = (twin.precondition(r).tobytes(), _solved(twin, b, p))
        twin.set_coef_mg(True)
        want = (twin.precondition(r).tobytes(), _solved(twin, b, p))
    finally:
        twin.close()
    cz = _handle(prec, args, state)
    try:
        cz.set_mg_lines(True)  # (before the coefficients: idle)
        assert cz.info()["mg_lines"] == 0
        cz.set_face_coef(*beta)
        assert cz.info()["mg_lines"] == 0
        assert (cz.precondition(r).tobytes(), _solved(cz, b, p)) == scaled
        cz.set_coef_mg(True)
        assert cz.info()["mg_lines"] == 1  # the flag is remembered
        lines = (cz.precondition(r).tobytes(), _solved(cz, b, p))
        assert lines[0] != want[0] and lines[1][1] != want[1][1]
        cz.set_mg_lines(False)
        assert cz.info()["mg_lines"] == 0 and cz.info()["coef_mg"] == 1
        assert (cz.precondition(r).tobytes(), _solved(cz, b, p)) == want
        cz.set_mg_lines(True)
        assert (cz.precondition(r).tobytes(), _solved(cz, b, p)) == lines
        cz.set_coef_mg(False)
        assert cz.info()["mg_lines"] == 0
        assert (cz.precondition(r).tobytes(), _solved(cz, b, p)) == scaled
    finally:
        cz.close()


# ---- PCG against the exact-dot restatement
@pytest.mark.parametrize("c", LP.PCG_CASES, ids=[c["id"] for c in LP.PCG_CASES])
def test_pcg_against_the_exact_dot_restatement(c):
    """K iterations: FP32 bit for bit (field and history), FP64 within 2 E + 8 ulp with the history within its envelope
    (tests/test_lines_oracle.py holds the premise of every case); the iteration count is K on both sides"""
    gsz, prec, state = c["gsz"], c["prec"], K.STATES[c["state"]]
    b, p, beta = LP.case_problem(c)
    cz = _handle(prec, list(gsz) + ["pcg", c["K"], c["coef"], c["pc"]], state)
    try:
        cz.set_eps(1e-30)
        _with_lines(cz, beta)
        cz.set_rhs(b)
        cz.set_field(p)
        itr = cz.solve()
        got, hist, info = cz.field(), cz.history(), cz.info()
    finally:
        cz.close()
    assert info["mg_lines"] == 1 and info["coef_mg"] == 1 and info["mg_cycles"] == c["K"]
    if prec == "f32":
        ref = LP.case_run(c)
        assert itr == ref.itr == c["K"]
        assert got.tobytes() == ref.P.tobytes(), c["id"]
        assert hist == [v for _, v in ref.history], c["id"]
    else:
        ref, E, Eh = LP.envelope_f64(gsz, c["pc"], c["coef"], state, c["K"], b, p, beta, eps=1e-30)
        assert itr == ref.itr == c["K"]
        ok, worst = PP.f64_close(got, ref.P, E)
        assert ok, (c["id"], worst)
        okh, worsth = PP.f64_close(hist, [v for _, v in ref.history], Eh)
        assert okh, (c["id"], worsth)


@pytest.mark.parametrize("field", ["stretch30", "anisoz100"])
def test_counts_are_the_recorded_ones(field):
    """(33, 47, 61) FP64 to eps 1e-8, mgrb 1.0: the restatement's recorded counts with lines in the three states"""
    g = LP.COUNT_BOX
    b, p = PP.problem(g, "f64", 0)
    got = {}
    for name in LP.COUNT_STATES:
        cz = _handle("f64", list(g) + ["pcg", 300, 1.0, "mgrb"], K.STATES[name])
        try:
            cz.set_eps(LP.COUNT_EPS)
            _with_lines(cz, LP.FIELDS[field](g, "f64"))
            cz.set_rhs(b)
            cz.set_field(p)
            got[name] = cz.solve()
        finally:
            cz.close()
    print(field, got)
    assert got == {name: LM.COUNTS[field, name][0] for name in LP.COUNT_STATES}


# ---- the state of the flag and the refusals
def test_idle_with_mg_jacobi_and_none():
    """accepted and idle where the smoother is not mgrb's: the solve is that of a handle without the flag"""
    gsz, prec = (9, 7, 12), "f64"
    b, p = PP.problem(gsz, prec, 1)
    beta = K.random(gsz, prec)
    for pc in ("mg", "jacobi", "none"):
        out = []
        for flag in (False, True):
            cz = _handle(prec, list(gsz) + ["pcg", 5, 0.8, pc])
            try:
                cz.set_face_coef(*beta)
                cz.set_coef_mg(True)
                if flag:
                    cz.set_mg_lines(True)
                assert cz.info()["mg_lines"] == 0 and cz.info()["coef_mg"] == (1 if pc == "mg" else 0)
                out.append(_solved(cz, b, p))
            finally:
                cz.close()
        assert out[0] == out[1] and out[0][0] == 5, pc


def test_refusals_the_cleared_state_and_the_coarse_overflow(capfd):
    from cubez_amd import CZ
    gsz, prec = (33, 47, 61), "f32"
    n = 0
    fresh = CZ(prec, quiet=True)
    try:
        assert fresh.lib.cz_set_mg_lines(fresh.h, 1) == 0  # before cz_setup
        n += 1
    finally:
        fresh.close()
    maf = _handle(prec, [9, 7, 12, "jacobi_maf", 50, 0.8])
    try:
        assert maf.lib.cz_set_mg_lines(maf.h, 1) == 0 and maf.info()["mg_lines"] == 0
        n += 1
    finally:
        maf.close()
    sz, idx, ins, r = TN._cycle_rhs(prec, gsz)
    beta = LP.stretch(gsz, prec, 30)
    over = _handle(prec, list(gsz) + ["pcg", 3, 1.2, "mgrb"])
    try:
        over.set_face_coef(*beta)
        over.set_coef_mg(True)
        before = over.precondition(r).tobytes()
        with pytest.raises(RuntimeError):
            over.set_mg_lines(True)  # coef 1.2
        n += 1
        assert over.lib.cz_set_mg_lines(over.h, 0) == 1  # (off is no request for lines)
        assert over.info()["mg_lines"] == 0 and over.info()["coef_mg"] == 1 and over.precondition(r).tobytes() == before
    finally:
        over.close()
    args = list(gsz) + ["pcg", 3, 1.0, "mgrb"]
    cz = _handle(prec, args)
    try:
        assert cz.lib.cz_set_mg_lines(cz.h, 2) == 0 and cz.lib.cz_set_mg_lines(cz.h, -1) == 0
        n += 2
        _with_lines(cz, beta)
        # cz_setup clears the flag
        assert cz.setup(args) == 1
        assert cz.info()["mg_lines"] == 0
        cz.set_face_coef(*beta)
        cz.set_coef_mg(True)
        assert cz.info()["mg_lines"] == 0 and cz.info()["coef_mg"] == 1
        points = cz.precondition(r).tobytes()
        cz.set_mg_lines(True)
        assert cz.info()["mg_lines"] == 1 and cz.precondition(r).tobytes() != points
        # the overflow of a coarse weight (tests/test_gpu_coefmg.py) drops the coefficient hierarchy: the lines go idle with it
        huge = [np.full(gsz, 1e37, dtype=np.float32) for _ in range(3)]
        with pytest.raises(RuntimeError):
            cz.set_face_coef(*huge)
        assert cz.info()["coef_mg"] == 0 and cz.info()["mg_lines"] == 0 and cz.info()["face_coef"] == 1
    finally:
        cz.close()
    err = capfd.readouterr().err
    assert err.count("cz_set_mg_lines: ") == n, err
    for why in ("cz_setup first", "MAF", "0 < coef <= 1", "indefinite", "the flag is 0 or 1"):
        assert why in err, why


def test_a_decomposed_run_is_refused(capfd):
    gsz = (32, 36, 40)

    def work(q):
        cz = _handle("f32", list(gsz) + ["pcg", 10, 0.8, "mg", 2, 1, 1])
        try:
            return cz.lib.cz_set_mg_lines(cz.h, 1), cz.info()["mg_lines"]
        finally:
            cz.close()

    assert TN._ranks("f32", (2, 1, 1), work) == [(0, 0)] * 2
    assert capfd.readouterr().err.count("cz_set_mg_lines: a decomposed run") == 2


# ---- Refined
def test_refined_with_lines():
    """stretch 30 at 64^3, Z faces zero-flux: the flag on both libraries (in force on the FP32 one, which preconditions with mgrb 1.0), the
    FP64 answer to 1e-10, in fewer inner iterations than with the point sweeps of the same inner solver"""
    from cubez_amd.refine import Refined
    _torch()
    gsz = (64, 64, 64)
    beta = LP.stretch(gsz, "f64", 30)
    b, p = PP.problem(gsz, "f64", 0)
    inner = {}
    for on in (True, False):
        r = Refined(gsz, inner=("pcg", 1000, 1.0, "mgrb"), neumann=K.STATES["inflow"][0])
        try:
            r.set_face_coef(*beta)
            r.set_coef_mg(True)
            r.set_mg_lines(on)
            assert r.lo.info()["mg_lines"] == int(on) and r.hi.info()["mg_lines"] == 0
            r.set_rhs(b)
            r.set_field(p)
            _, ss0 = r.hi.get_residual()
            steps = r.solve(tol=1e-10)
            hist = list(r.history)
            _, ss1 = r.hi.get_residual()
            inner[on] = sum(h[2] for h in hist)
            r.set_mg_lines(False)
            assert r.lo.info()["mg_lines"] == 0
        finally:
            r.close()
        print("lines", on, "outer steps", steps, "inner iterations", inner[on], hist)
        assert steps > 0 and hist[-1][1] <= 1e-10 and np.sqrt(ss1) <= 1e-10 * np.sqrt(ss0), hist
    assert inner[True] < inner[False], inner
    with pytest.raises(RuntimeError):
        r2 = Refined(gsz)  # the default inner solver relaxes with 1.2
        try:
            r2.set_mg_lines(True)
        finally:
            assert r2.lo.info()["mg_lines"] == 0 and r2.hi.info()["mg_lines"] == 0
            r2.close()
