"""The zebra line smoother along Z on the CPU: the numpy restatement of tests/lines_parity.py against the properties the
smoother rests on -- a swept row solves its tridiagonal system, a folded end is the row of the zero-flux operator, the from-zero forms, a
symmetric definite preconditioner at omega = 1 (and an indefinite one at 1.2 with a periodic Z: the reason of the refusal) -- its recorded
iteration counts, the premises of the GPU cases of tests/test_gpu_lines.py, and the new entries at the library boundary."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coef_parity as K  # noqa: E402
import coefmg_parity as G  # noqa: E402
import lines_measured as LM  # noqa: E402
import lines_parity as LP  # noqa: E402
import mg_parity as M  # noqa: E402
import problem_parity as PP  # noqa: E402
import project_parity as J  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIX = ("dirichlet", "inflow", "closed", "channel", "triple", "px")
SMALL = [(9, 7, 12), (5, 5, 40)]
SMALL_IDS = ["9x7x12", "5x5x40"]


def _tridiagonal(L, d, j, i):
    """row (i, j)'s system as a dense matrix in double: a_K = Z(K-1), d_K, c_K = Z(K)"""
    Z = L.W[2][j, i].astype(np.float64)
    n = d.shape[2]
    T = np.diag(d[j, i].astype(np.float64))
    for k in range(n - 1):
        T[k, k + 1] = Z[k + 1]
        T[k + 1, k] = Z[k + 1]
    return T


# ---- one sweep
def test_a_swept_row_satisfies_its_system_exactly_where_every_pivot_divides():
    """a hand-made level in double whose pivots are all -8: Z = 2 on every link, X = Y = 1 at K = 0 and 1.125 above (D = 8, then 8.5 =
    8 + 2 * 2 / 8), small integers in b and u.  cp = -0.25 throughout and every quotient is a division by 8, so each of the 10 cells adds
    three fractional bits and nothing is rounded in double: T y = f holds exactly on the swept rows, and x = y at omega = 1"""
    nj, ni, nk = 3, 4, 10
    w = np.where(np.arange(nk) == 0, 1.0, 1.125)
    X = np.broadcast_to(w, (nj, ni + 1, nk)).copy()
    Y = np.broadcast_to(w, (nj + 1, ni, nk)).copy()
    Z = np.full((nj, ni, nk + 1), 2.0)
    L = G.Level([X, Y, Z], (0,) * 6, (0,) * 3)
    assert np.array_equal(L.D[0, 0], np.where(np.arange(nk) == 0, 8.0, 8.5))
    rng = np.random.default_rng(3)
    b = rng.integers(-8, 9, size=L.shape).astype(np.float64)
    u = rng.integers(-8, 9, size=L.shape).astype(np.float64)
    f, d = LP.line_system(u, b, L)
    for c in (0, 1):
        x = LP.line_sweep(u, b, L, 1.0, c)
        colour = LP.row_colour(L.shape)[:, :, 0]
        for j in range(nj):
            for i in range(ni):
                if colour[j, i] != c:
                    assert x[j, i].tobytes() == u[j, i].tobytes()
                else:
                    assert np.array_equal(_tridiagonal(L, d, j, i) @ x[j, i], f[j, i]), (j, i)


@pytest.mark.parametrize("name", SIX)
def test_a_swept_row_satisfies_its_tridiagonal_system(name):
    """FP32 sweeps of every level of (9, 7, 12) at omega = 1 under `random`: every row of the swept colour holds the solution of its system,
    within 4 ulp (FP32, of the row's largest value) of a dense solve in double; the rows of the other colour keep their bytes.
    (The forward error of the elimination is a few ulp times the row system's condition number.  With faces in [0.5, 2] the X / Y links on
    the diagonal are at least half the Z links beside it at level 0, and a coarse weight sums two to four fine ones in every direction
    alike, so the row systems stay well conditioned and 4 ulp is a bar; on a stretched field the condition number is of the order of the
    stretch, and the exact case above stands for it)"""
    gsz, state = (9, 7, 12), K.STATES[name]
    H = G.hierarchy(K.random(gsz, "f32"), gsz, state)
    rng = np.random.default_rng(7)
    for l, L in enumerate(H):
        if not LP.has_lines(L):
            continue
        b = rng.standard_normal(L.shape).astype(np.float32)
        u = rng.standard_normal(L.shape).astype(np.float32)
        f, d = LP.line_system(u, b, L)
        for c in (0, 1):
            x = LP.line_sweep(u, b, L, 1.0, c)
            colour = LP.row_colour(L.shape)[:, :, 0]
            for j in range(L.shape[0]):
                for i in range(L.shape[1]):
                    if colour[j, i] != c:
                        assert x[j, i].tobytes() == u[j, i].tobytes()
                        continue
                    want = np.linalg.solve(_tridiagonal(L, d, j, i), f[j, i].astype(np.float64))
                    ulp = np.spacing(np.float32(np.abs(want).max()))
                    assert np.abs(x[j, i] - want).max() <= 4 * ulp, (l, j, i)


@pytest.mark.parametrize("name", SIX)
def test_the_row_systems_are_the_operator_and_a_folded_end_is_the_zero_flux_row(name):
    """for any u, f(u) - T u is the level's residual b - A u at every point, in double: the X / Y links and the unfolded ends on the right,
    the Z links and the folded ends in T.  On a zero-flux Z face of level 0 the end is folded: the diagonal there is -(D - Z(face)), the
    row of the operator whose ghost equals the end cell, and no ghost term stands on the right"""
    gsz, state = (9, 7, 12), K.STATES[name]
    H = G.hierarchy(LP.stretch(gsz, "f64", 30), gsz, state)
    rng = np.random.default_rng(11)
    for l, L in enumerate(H):
        lo, hi = LP.folded(L)
        assert (lo, hi) == ((bool(state[0][4]), bool(state[0][5])) if l == 0 and not state[1][2] else (False, False))
        b = rng.standard_normal(L.shape)
        u = rng.standard_normal(L.shape)
        f, d = LP.line_system(u, b, L)
        Z = L.W[2]
        if lo:
            assert np.array_equal(d[:, :, 0], -L.D[:, :, 0] + Z[:, :, 0])
        if hi:
            assert np.array_equal(d[:, :, -1], -L.D[:, :, -1] + Z[:, :, -1])
        Tu = d * u
        Tu[:, :, 1:] += Z[:, :, 1:-1] * u[:, :, :-1]
        Tu[:, :, :-1] += Z[:, :, 1:-1] * u[:, :, 1:]
        r = G.residual(u, b, L)
        assert np.abs((f - Tu) - r).max() <= 1e-12 * np.abs(r).max(), l


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", list(K.PCG_STATES))
def test_from_zero_forms_equal_sweeps_of_a_cleared_array(name, prec):
    """every level of (33, 47, 61): the first colour from zero (b, D, Z only) and the second colour (its own row and Z ghosts literal zeros)
    give the bytes of the general form on a cleared array, forward and backward"""
    gsz, state = (33, 47, 61), K.STATES[name]
    for field in ("random", "stretch30"):
        H = G.hierarchy(LP.FIELDS[field](gsz, prec), gsz, state)
        for l, L in enumerate(H):
            if not LP.has_lines(L):
                continue
            b = np.random.default_rng(50 + l).standard_normal(L.shape).astype(K._real(prec))
            for omg in (1.0, 0.8):
                for post in (False, True):
                    first = 1 if post else 0
                    one = LP.line_sweep(None, b, L, omg, first, mode=1)
                    gen = LP.line_sweep(np.zeros_like(b), b, L, omg, first)
                    assert one.tobytes() == gen.tobytes(), (l, post)
                    two = LP.line_sweep(one, b, L, omg, 1 - first, mode=2)
                    assert two.tobytes() == LP.line_sweep(gen, b, L, omg, 1 - first).tobytes(), (l, post)
                    assert two.tobytes() == LP.pair_from_zero_forms(b, L, omg, post).tobytes()


# ---- the preconditioner
def _fields(gsz):
    return {"random": K.random(gsz, "f64"), "bubble1000": K.bubble(gsz, "f64", 1000), "stretch30": LP.stretch(gsz, "f64", 30)}


@pytest.mark.parametrize("name", SIX)
@pytest.mark.parametrize("gsz", SMALL, ids=SMALL_IDS)
def test_preconditioner_is_symmetric_and_definite_at_omega_one(gsz, name):
    """M^-1 of the line cycle assembled column by column: symmetric within 1e-12 of max |M^-1| (the bar leaves room for another summation
    order and for nothing else), its symmetric part negative definite"""
    state = K.STATES[name]
    assert J.fits(gsz, state)
    for field, beta in _fields(gsz).items():
        Mi = LP.inverse(G.hierarchy(beta, gsz, state), gsz, 1.0)
        asym = np.abs(Mi - Mi.T).max() / np.abs(Mi).max()
        top = np.linalg.eigvalsh(0.5 * (Mi + Mi.T))[-1]
        print(gsz, name, field, "asymmetry", asym, "largest eigenvalue", top)
        assert asym <= 1e-12, (field, asym)
        assert top < 0, (field, top)


def test_over_relaxed_lines_with_a_periodic_z_are_not_definite():
    """omega = 1.2, channel, stretch 30 on (9, 7, 12): the lagged wrap of the periodic Z makes M^-1 indefinite -- why cz_set_mg_lines refuses
    a coefficient above 1"""
    gsz = (9, 7, 12)
    Mi = LP.inverse(G.hierarchy(LP.stretch(gsz, "f64", 30), gsz, K.STATES["channel"]), gsz, 1.2)
    top = np.linalg.eigvalsh(0.5 * (Mi + Mi.T))[-1]
    print("largest eigenvalue", top)
    assert top > 0


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_levels_of_one_row_keep_the_point_sweeps(prec):
    """(5, 5, 40) closed comes down to levels with ni = nj = 1, whose single line is the whole singular operator (last pivot 0): they keep
    the point colour sweeps and the cycle runs without a floating-point exception"""
    gsz, state = (5, 5, 40), K.STATES["closed"]
    H = G.hierarchy(LP.stretch(gsz, prec, 30), gsz, state)
    lone = [l for l, L in enumerate(H) if not LP.has_lines(L)]
    assert lone and lone[0] >= 1 and all(H[l].shape[:2] == (1, 1) for l in lone)
    sz, idx = K.box(gsz)
    r = np.zeros((gsz[1] + 4, gsz[0] + 4, gsz[2] + 4), dtype=K._real(prec))
    ins = M.inner(sz, idx)
    r[ins] = np.random.default_rng(23).standard_normal(r[ins].shape).astype(r.dtype)
    with np.errstate(all="raise"):
        z = LP.apply(H, r, sz, idx, 1.0)
    assert np.isfinite(z).all() and z[ins].any()
    # the lone level's line system itself: its last pivot vanishes
    L = H[lone[0]]
    f, d = LP.line_system(np.zeros(L.shape, dtype=r.dtype), np.ones(L.shape, dtype=r.dtype), L)
    assert np.array_equal(-d[0, 0], L.W[2][0, 0, 1:] + L.W[2][0, 0, :-1]) and L.W[2][0, 0, 0] == 0 and L.W[2][0, 0, -1] == 0


# ---- counts
def test_ones_gives_finite_results_and_its_recorded_count():
    g = LP.COUNT_BOX
    b, p = PP.problem(g, "f64", 0)
    r = LP.run(list(g), "mgrb", 1.0, "f64", K.STATES["dirichlet"], 300, b, p, K.ones(g, "f64"), eps=LP.COUNT_EPS)
    print("ones", r.itr)
    assert np.isfinite(r.P).all() and np.isfinite([v for _, v in r.history]).all()
    assert r.itr == LM.ONES


@pytest.mark.parametrize("state", LP.COUNT_STATES)
@pytest.mark.parametrize("field", LP.COUNT_FIELDS)
def test_iteration_counts_are_the_recorded_ones(field, state):
    """33 x 47 x 61, FP64, eps 1e-8: lines at coef 1.0 and point colour sweeps at coef 1.2, both with the coefficient hierarchy, re-measured;
    on the stretched fields lines need a third of the iterations at most, on `random` at most one more"""
    got = (LP.count(field, state, True), LP.count(field, state, False))
    print(field, state, got)
    assert got == LM.COUNTS[field, state]
    lines, points = got
    if field == "random":
        assert lines <= points + 1
    else:
        assert 3 * lines <= points


# ---- the premises of the GPU cases
@pytest.mark.parametrize("c", LP.PCG_CASES, ids=[c["id"] for c in LP.PCG_CASES])
def test_premise_of_the_gpu_pcg_cases(c):
    """FP32: no dot within its summation bound of a rounding boundary (closed states: the sums too); FP64: the envelope of the runs with
    every dot at either edge of its bound stays below 1e-8"""
    b, p, beta = LP.case_problem(c)
    state = K.STATES[c["state"]]
    if c["prec"] == "f32":
        r = LP.premise_f32(c["gsz"], c["pc"], c["coef"], state, c["K"], b, p, beta, eps=1e-30)
    else:
        r, E, Eh = LP.envelope_f64(c["gsz"], c["pc"], c["coef"], state, c["K"], b, p, beta, eps=1e-30)
        print(c["id"], "envelope", float(E.max()), float(Eh.max()))
        assert E.max() <= 1e-8 and Eh.max() <= 1e-8
    assert r.itr == c["K"] and len(r.history) == c["K"] and r.cycles == c["K"]


def test_the_gpu_pcg_cases_cover_every_state_and_precision():
    for key, want in (("state", set(K.PCG_STATES)), ("prec", {"f32", "f64"}), ("field", {"random", "stretch30"}), ("pc", {"mgrb"})):
        assert {c[key] for c in LP.PCG_CASES} == want, key
    assert all(0 < c["coef"] <= 1 for c in LP.PCG_CASES)


# ---- the library boundary
NEW = ("cz_set_mg_lines", "czhip_mg_set_lines", "czhip_mg_line_chunk")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_libraries_export_the_entries(prec):
    from cubez_amd import lib
    so = ctypes.CDLL(lib.lib_path(prec))
    assert all(hasattr(so, name) for name in NEW)
    so.czhip_mg_line_chunk.restype = ctypes.c_int
    c = so.czhip_mg_line_chunk()
    assert c >= 2 and c % (16 // (4 if prec == "f32" else 8)) == 0  # whole 16-byte vectors
    so.czhip_mg_set_lines.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert so.czhip_mg_set_lines(None, 1) == 0  # a NULL handle: refused, nothing touched


def test_header_declares_them_and_python_lists_them():
    from cubez_amd import lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cz_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+cz_set_mg_lines\s*\(\s*cz_handle\s*\*\s*,\s*int\s+\w*\s*\)", src)
    assert re.search(r"int\s+czhip_mg_set_lines\s*\(\s*cz_mg\s*\*\s*\w*\s*,\s*int\s+\w*\s*\)", src)
    assert re.search(r"int\s+czhip_mg_line_chunk\s*\(\s*void\s*\)", src)
    assert all(name in lib.ABI_SYMBOLS for name in NEW)
    # no new timing label: the line kernel runs under the labels of the colour sweeps it replaces
    assert len(lib.LABELS) == 23 and all(n in lib.LABELS for n in ("rbsor", "mg_rb"))


def test_the_driver_classes_have_the_method():
    import inspect
    from cubez_amd import CZ
    from cubez_amd.refine import Refined
    assert callable(getattr(CZ, "set_mg_lines", None)) and callable(getattr(Refined, "set_mg_lines", None))
    src = inspect.getsource(CZ.info)
    assert '"mg_lines"' in src and src.index('"coef_mg"') < src.index('"mg_lines"')
