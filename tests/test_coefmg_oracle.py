"""Face coefficients inside the multigrid hierarchy on the CPU: the numpy restatement of tests/coefmg_parity.py against
the constant restatement (unit coefficients: the same bytes), against the properties the construction rests on -- the exact Galerkin
product, a symmetric definite preconditioner -- its recorded iteration counts, the premises of the GPU cases of tests/test_gpu_coefmg.py,
and the new entries at the library boundary."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coef_parity as K  # noqa: E402
import coefmg_measured as CM  # noqa: E402
import coefmg_parity as G  # noqa: E402
import mg_parity as M  # noqa: E402
import neumann_parity as N  # noqa: E402
import periodic_parity as P  # noqa: E402
import problem_parity as PP  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BOXES = [(9, 7, 12), (33, 47, 61)]
BOX_IDS = ["x".join(map(str, g)) for g in BOXES]
RUNS = [("mg", 0.8), ("mgrb", 1.2)]
SINGULAR = ("closed", "channel")


def _rhs(prec, gsz, seed=23):
    sz, idx = K.box(gsz)
    r = np.zeros((gsz[1] + 4, gsz[0] + 4, gsz[2] + 4), dtype=K._real(prec))
    ins = M.inner(sz, idx)
    r[ins] = np.random.default_rng(seed).standard_normal(r[ins].shape).astype(r.dtype)
    return sz, idx, ins, r


# ---- unit coefficients: the constant cycle
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", list(K.PCG_STATES))
@pytest.mark.parametrize("gsz", BOXES + [(4, 9, 12)], ids=BOX_IDS + ["4x9x12"])
def test_ones_cycle_is_the_constant_cycle(gsz, name, prec):
    """beta = 1: the bytes of periodic_parity.apply (level 0 through the oracle's C kernels) for both smoothers; (4, 9, 12): a periodic
    direction that comes down to one point"""
    state = K.STATES[name]
    sz, idx, ins, r = _rhs(prec, gsz)
    H = G.hierarchy(K.ones(gsz, prec), gsz, state)
    for kind, omg in RUNS:
        ref = P.apply(kind, P.kernels(prec, state[0], state[1]), r, sz, idx, omg)[ins]
        got = G.apply(kind, H, r, sz, idx, omg)[ins]
        assert ref.any() and got.tobytes() == ref.tobytes(), kind


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", list(K.PCG_STATES))
@pytest.mark.parametrize("gsz", BOXES, ids=BOX_IDS)
def test_ones_pcg_is_the_scaled_run(gsz, name, prec):
    """beta = 1: s = 1 exactly, and three iterations of PCG with the coefficient cycle give the field and the history of the scaled run"""
    state = K.STATES[name]
    b, p = PP.problem(gsz, prec, 0)
    beta = K.ones(gsz, prec)
    for pc, coef in RUNS:
        on = G.run(gsz, pc, coef, prec, state, 3, b, p, beta, eps=1e-30)
        off = K.run(gsz, pc, coef, prec, state, 3, b, p, beta, eps=1e-30)
        assert on.itr == off.itr == 3 and on.cycles == 3
        assert on.P.tobytes() == off.P.tobytes() and on.history == off.history, pc


@pytest.mark.parametrize("name", list(K.PCG_STATES))
@pytest.mark.parametrize("gsz", BOXES + [(4, 9, 12)], ids=BOX_IDS + ["4x9x12"])
def test_ones_weights_are_the_integers_of_the_constant_hierarchy(gsz, name):
    """every level >= 1: the links are mg_parity.weights (0 where the level has no link across a box face), the diagonal the masked one of
    periodic_parity's levels (mg_links)"""
    state = K.STATES[name]
    faces, per, _ = state
    R = np.float32
    H = G.hierarchy(K.ones(gsz, "f32"), gsz, state)
    n0 = M.n0_of(K.box(gsz)[1])
    assert len(H) == len(M.level_dims(n0))
    for l in range(1, len(H)):
        mask, wraps = P.level_state(n0, l, faces, per)
        w = N.weights(n0, l, R, mask)
        assert np.array_equal(H[l].D, w[3]) and H[l].wraps == tuple(wraps)
        for d in range(3):
            up, dn = G._take(H[l].W[d], d, slice(1, None)).copy(), G._take(H[l].W[d], d, slice(None, -1)).copy()
            for a, sel, cut in ((up, -1, mask[2 * d + 1]), (dn, 0, mask[2 * d])):
                if cut:
                    assert not G._take(a, d, sel).any()
                    G._take(a, d, sel)[...] = G._take(w[d], d, sel)
                assert np.array_equal(a, w[d]), (l, d)


# ---- the Galerkin product
@pytest.mark.parametrize("name", list(K.PCG_STATES))
def test_galerkin_identity_is_exact_in_integers(name):
    """integer coefficients 1 .. 4 on (9, 7, 12): the assembled level-l operator equals P^T A_{l-1} P exactly at every level; row sums are
    exactly zero in the singular states"""
    gsz, state = (9, 7, 12), K.STATES[name]
    H = G.hierarchy(K.ints(gsz, "f64"), gsz, state)
    assert len(H) == 3 and G.count_bad(H) == 0
    A = [G.level_operator(L) for L in H]
    assert np.array_equal(A[0], K.assembled(gsz, K.ints(gsz, "f64"), state))
    for l in range(1, len(H)):
        Pm = G.aggregation(H[l - 1].shape)
        assert np.array_equal(A[l], Pm.T @ A[l - 1] @ Pm), l
        assert np.array_equal(A[l], A[l].T)
    for Al in A:
        rows = Al.sum(axis=1)
        if name in SINGULAR:
            assert np.array_equal(rows, np.zeros_like(rows))
        else:
            assert rows.max() <= 0 and rows.min() < 0


@pytest.mark.parametrize("field", ["random", "bubble100"])
@pytest.mark.parametrize("pc,coef", RUNS)
@pytest.mark.parametrize("name", ["dirichlet", "inflow"])
def test_preconditioner_is_symmetric_and_definite(name, pc, coef, field):
    """M_beta^-1 applied to the unit vectors of (9, 7, 12): symmetric to rounding (the tolerance of the scaled preconditioner's check) and
    definite with the sign of the operator"""
    gsz, state = (9, 7, 12), K.STATES[name]
    sz, idx = K.box(gsz)
    ins = M.inner(sz, idx)
    H = G.hierarchy(K.FIELDS[field](gsz, "f64"), gsz, state)
    n = [v - 2 for v in gsz]
    nn = n[0] * n[1] * n[2]
    Mi = np.zeros((nn, nn))
    for q in range(nn):
        e = np.zeros(tuple(gsz))
        e[1 + q // (n[1] * n[2]), 1 + (q // n[2]) % n[1], 1 + q % n[2]] = 1.0
        z = G.apply(pc, H, PP.pad(e), sz, idx, coef)
        Mi[:, q] = PP.unpad(z)[1:-1, 1:-1, 1:-1].ravel()
        assert not PP.unpad(z)[0].any() and z[ins].any()
    assert np.abs(Mi - Mi.T).max() <= 1e-13 * np.abs(Mi).max()
    assert np.linalg.eigvalsh(0.5 * (Mi + Mi.T))[-1] < 0


# ---- the forms of the kernels
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", list(K.PCG_STATES))
def test_from_zero_forms_equal_a_sweep_from_a_cleared_array(name, prec):
    """every level of (33, 47, 61): the from-zero sweep (b and D only) and the from-zero colour sweeps give the bytes of the general form on zeros"""
    gsz, state = (33, 47, 61), K.STATES[name]
    H = G.hierarchy(K.random(gsz, prec), gsz, state)
    for l, L in enumerate(H):
        b = np.random.default_rng(50 + l).standard_normal(L.shape).astype(K._real(prec))
        zero = np.zeros_like(b)
        for omg in (0.8, 1.2):
            assert G.sweep(None, b, L, omg).tobytes() == G.sweep(zero, b, L, omg).tobytes(), l
            for c in (0, 1):
                first = G.colour_sweep(None, b, L, omg, c)
                assert first.tobytes() == G.colour_sweep(zero, b, L, omg, c).tobytes(), (l, c)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", list(K.PCG_STATES))
def test_level_path_equals_tail_path(name, prec):
    """the recursion of mg_walk from level t and the loops of the one-workgroup tail give the same bytes, for every t"""
    gsz, state = (33, 47, 61), K.STATES[name]
    R = K._real(prec)
    H = G.hierarchy(K.bubble(gsz, prec, 1000), gsz, state)
    for kind, omg in RUNS:
        for t in range(1, len(H)):
            b = np.random.default_rng(60 + t).standard_normal(H[t].shape).astype(R)
            assert G.vcycle(b, t, H, R(omg), kind).tobytes() == G.tail(b, t, H, R(omg), kind).tobytes(), (kind, t)


def test_a_coarse_overflow_is_counted():
    """FP32, faces of 1e37: every level-0 weight and diagonal is finite, a coarse level overflows; FP64 has room; the stored zeros of the
    dropped links are not counted"""
    gsz = (33, 47, 61)
    huge = [np.full(gsz, 1e37, dtype=np.float32) for _ in range(3)]
    with np.errstate(over="ignore"):
        H = G.hierarchy(huge, gsz, K.STATES["dirichlet"])
    assert np.isfinite(H[0].D).all() and all(np.isfinite(w).all() for w in H[0].W)
    assert G.count_bad(H) > 0 and not np.isfinite(H[-1].D).all()
    assert G.count_bad(G.hierarchy([a.astype(np.float64) for a in huge], gsz, K.STATES["dirichlet"])) == 0
    for name in K.PCG_STATES:
        Hs = G.hierarchy(K.random(gsz, "f32"), gsz, K.STATES[name])
        assert G.count_bad(Hs) == 0, name
        if name == "closed":
            assert all(not G._take(L.W[d], d, s).any() for L in Hs[1:] for d in range(3) for s in (0, -1))


# ---- counts
@pytest.mark.parametrize("pc,coef", K.COUNT_RUNS)
def test_iteration_counts_are_the_recorded_ones(pc, coef):
    """33 x 47 x 61, FP64, Dirichlet, eps 1e-8, every field: the recorded counts re-measured, and against the scaled preconditioner --
    `ones` needs the constant operator's count, no field needs more than scaled, bubble1000 at most half of scaled"""
    g = K.COUNT_BOX
    b, p = PP.problem(g, "f64", 0)
    st = K.STATES["dirichlet"]
    got = {f: G.run(list(g), pc, coef, "f64", st, 300, b, p, K.FIELDS[f](g, "f64"), eps=K.COUNT_EPS).itr for f in K.FIELDS}
    print(pc, got)
    assert got == {f: CM.COUNTS[f, pc] for f in K.FIELDS}
    scaled = {f: K.COUNTS[f, pc][1] for f in K.FIELDS if (f, pc) in K.COUNTS}
    for f in ("random",):
        scaled[f] = G.run(list(g), pc, coef, "f64", st, 300, b, p, K.FIELDS[f](g, "f64"), eps=K.COUNT_EPS, on=False).itr
        assert scaled[f] == CM.SCALED[f, pc]
    scaled["ones"] = K.COUNTS["constant", pc][1]
    assert set(scaled) == set(K.FIELDS)
    assert got["ones"] == scaled["ones"]
    for f in K.FIELDS:
        assert got[f] <= scaled[f], (f, got[f], scaled[f])
    assert 2 * got["bubble1000"] <= scaled["bubble1000"]


# ---- the premises of the GPU cases
@pytest.mark.parametrize("c", G.PCG_CASES, ids=[c["id"] for c in G.PCG_CASES])
def test_premise_of_the_gpu_pcg_cases(c):
    """FP32: no dot within its summation bound of a rounding boundary (closed states: the sums too); FP64: the envelope of the runs with
    every dot at either edge of its bound stays below 1e-8"""
    b, p, beta = G.case_problem(c)
    state = K.STATES[c["state"]]
    if c["prec"] == "f32":
        r = G.premise_f32(c["gsz"], c["pc"], c["coef"], state, c["K"], b, p, beta, eps=1e-30)
    else:
        r, E, Eh = G.envelope_f64(c["gsz"], c["pc"], c["coef"], state, c["K"], b, p, beta, eps=1e-30)
        print(c["id"], "envelope", float(E.max()), float(Eh.max()))
        assert E.max() <= 1e-8 and Eh.max() <= 1e-8
    assert r.itr == c["K"] and len(r.history) == c["K"] and r.cycles == c["K"]


def test_the_gpu_pcg_cases_cover_every_state_smoother_and_precision():
    for key, want in (("state", set(K.PCG_STATES)), ("pc", {"mg", "mgrb"}), ("prec", {"f32", "f64"}),
                      ("gsz", {(9, 7, 12), (33, 47, 61), (40, 40, 1100)})):
        assert {c[key] for c in G.PCG_CASES} == want, key


# ---- the library boundary
NEW = ("cz_set_coef_mg", "czhip_mg_set_coef")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_libraries_export_the_entries(prec):
    from cubez_amd import lib
    so = ctypes.CDLL(lib.lib_path(prec))
    assert all(hasattr(so, name) for name in NEW)


def test_header_declares_them_and_python_lists_them():
    from cubez_amd import lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cz_hip.h")).read(), flags=re.S)
    real = r"\s*const\s+CZ_REAL\s*\*\s*\w*\s*"
    assert re.search(r"int\s+cz_set_coef_mg\s*\(\s*cz_handle\s*\*\s*,\s*int\s+\w*\s*\)", src)
    assert re.search(r"int\s+czhip_mg_set_coef\s*\(\s*cz_mg\s*\*\s*\w*\s*,(" + real + r",){2}" + real + r"\)", src)
    assert all(name in lib.ABI_SYMBOLS for name in NEW)
    # no new timing label: the new kernels run under the labels of the constant cycle's kernels
    assert len(lib.LABELS) == 23 and all(n in lib.LABELS for n in ("jacobi", "rbsor", "mg_smooth", "mg_rb", "mg_restrict", "mg_tail", "mg_prolong"))


def test_the_driver_classes_have_the_method():
    from cubez_amd import CZ
    from cubez_amd.refine import Refined
    assert callable(getattr(CZ, "set_coef_mg", None)) and callable(getattr(Refined, "set_coef_mg", None))
    import inspect
    assert '"coef_mg"' in inspect.getsource(CZ.info)
