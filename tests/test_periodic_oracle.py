"""Periodic directions for pcg on the CPU (tests/periodic_parity.py): without a flag the restatement is that of
tests/neumann_parity.py and tests/closed_parity.py byte for byte; the filled kernels state the assembled periodic operator; the level
operators, as the rules state them, are the Galerkin products; the V-cycles with wrapped levels stay symmetric definite preconditioners,
red-black on odd periodic extents included; PCG converges in the iteration counts the GPU test expects; and the GPU cases of
tests/test_gpu_periodic.py satisfy the premises of their bars."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cg_parity as CP  # noqa: E402
import closed_parity as C  # noqa: E402
import mg_parity as M  # noqa: E402
import neumann_parity as N  # noqa: E402
import periodic_parity as P  # noqa: E402
import problem_parity as PP  # noqa: E402
import test_mg_decomp_oracle as TD  # noqa: E402
import test_mg_oracle as TM  # noqa: E402
from cubez_amd import decomp as D  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

KINDS = [("mg", 0.8), ("mgrb", 0.8), ("mgrb", 1.0), ("mgrb", 1.2)]
CF = [1, 1, 1, 1, 1, 1, 6]
SMALL = (9, 7, 12)


def _apply(kind, state, sz, idx, v_inner, omg):
    k = P.kernels("f64", state[0], state[1])
    r = k.alloc(sz)
    ins = M.inner(sz, idx)
    r[ins] = v_inner
    return P.apply(kind, k, r, sz, idx, omg)[ins]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_no_flag_is_the_existing_restatement(prec):
    """no periodic direction: the bytes of neumann_parity.run (a mask, and none) and of closed_parity.run, and of the V-cycles"""
    gsz = (9, 7, 12)
    b, p = PP.problem(gsz, prec, 0)
    for pc, coef in (("none", 0.8), ("jacobi", 0.8), ("mg", 0.8), ("mgrb", 1.2)):
        for faces in (N.NONE, N.FIVE):
            a, ref = P.run(gsz, pc, coef, prec, (faces, P.NOPER, False), 4, b, p, eps=1e-30), N.run(gsz, pc, coef, prec, faces, 4, b, p, eps=1e-30)
            assert a.itr == ref.itr and a.history == ref.history and a.P.tobytes() == ref.P.tobytes(), (pc, faces)
        a, ref = P.run(gsz, pc, coef, prec, (C.SIX, P.NOPER, True), 4, b, p, eps=1e-30), C.run(gsz, pc, coef, prec, 4, b, p, eps=1e-30)
        assert a.itr == ref.itr and a.history == ref.history and a.P.tobytes() == ref.P.tobytes() and a.means == ref.means, pc
    sz, idx, _ = TM._box((33, 47, 61))
    k, k0 = P.kernels(prec, N.FIVE, P.NOPER), N.Kernels("oracle", prec)
    k0.faces = N.FIVE
    r = k.alloc(sz)
    ins = M.inner(sz, idx)
    r[ins] = np.random.default_rng(1).standard_normal(r[ins].shape).astype(k.real)
    for kind in ("mg", "mgrb"):
        assert P.apply(kind, k, r, sz, idx, 0.8).tobytes() == N.apply(kind, k0, r, sz, idx, 0.8, N.FIVE).tobytes(), kind
    assert M.pad is not P.wrapped_pad and M.weights is N._UNMASKED_WEIGHTS


def test_the_seam_link_fails_without_the_rule():
    """the feature on the CPU: with a periodic direction the level operators differ from the unperiodic ones exactly by the seam links, at
    level 0 (the wrap) and at levels >= 1 (the wrapped ghost layer)"""
    n0 = tuple(v - 2 for v in SMALL)
    for level in range(len(M.level_dims(n0))):
        plain, per = P.level_operator(n0, level, N.NONE, P.NOPER), P.level_operator(n0, level, N.NONE, P.PX)
        dims = M.level_dims(n0)[level]
        diff = per - plain
        assert np.count_nonzero(diff) == 2 * dims[1] * dims[2] and (diff[diff != 0] > 0).all(), level  # (a link is + W)
    A0 = P.level_operator(n0, 0, N.NONE, P.PX)
    assert np.array_equal(A0, P.assembled(SMALL, N.NONE, P.PX))


@pytest.mark.parametrize("s", list(P.STATES))
def test_filled_calc_ax_is_the_assembled_operator(s):
    """the oracle's blas_calc_ax on a filled field = A u with A assembled entry by entry (7 x 5 x 10 inner cells, zero Dirichlet values); A is
    symmetric, its row sums are zero exactly when no Dirichlet face remains, and it is negative definite otherwise"""
    faces, per, closed = P.STATES[s]
    k = P.kernels("f64", faces, per)
    sz, idx, _ = TM._box(SMALL)
    ins = M.inner(sz, idx)
    u, au = k.alloc(sz), k.alloc(sz)
    u[ins] = np.random.default_rng(2).standard_normal(u[ins].shape)
    k.blas_calc_ax(au, u, sz, idx, np.array(CF, dtype=np.float64))
    A = P.assembled(SMALL, faces, per)
    v = PP.unpad(u)[1:-1, 1:-1, 1:-1].ravel()
    got = PP.unpad(au)[1:-1, 1:-1, 1:-1].ravel()
    assert np.abs(got - A @ v).max() <= 64 * np.finfo(np.float64).eps * np.abs(v).max()
    assert np.abs(A - A.T).max() == 0.0
    singular = not P.solvable(faces, per, False)
    assert singular == closed and (np.abs(A.sum(1)).max() == 0.0) == singular
    ev = np.linalg.eigvalsh(A)
    assert ev.max() < 1e-12 and (abs(ev.max()) < 1e-12) == singular and ev[-2] < -1e-3
    r, b = k.alloc(sz), k.alloc(sz)
    k.blas_calc_rk(r, u, b, sz, idx, np.array(CF, dtype=np.float64))
    assert np.abs(PP.unpad(r)[1:-1, 1:-1, 1:-1].ravel() + A @ v).max() <= 64 * np.finfo(np.float64).eps * np.abs(v).max()


@pytest.mark.parametrize("s", list(P.STATES))
@pytest.mark.parametrize("gsz", [(9, 7, 12), (4, 9, 12)], ids=["9x7x12", "4x9x12"])
def test_level_operators_are_the_galerkin_products(gsz, s):
    """levels 1 and 2 as the rules state them (wrapped ghost layers, the per-level mask) = P^T A P assembled densely, exactly (small
    integers).  (9, 7, 12): odd extents, an extent of 2 in x and y at level 2; (4, 9, 12): two points in x at level 0, one from level 1 on"""
    faces, per, _ = P.STATES[s]
    n0 = tuple(v - 2 for v in gsz)
    A = P.assembled(gsz, faces, per)
    dims = M.level_dims(n0)
    assert len(dims) == 3
    for level in (1, 2):
        Pm = P.prolongation(n0, level)
        assert np.array_equal(P.level_operator(n0, level, faces, per), Pm.T @ A @ Pm), (level, dims[level])
    if gsz == (4, 9, 12):
        assert dims[0][0] == 2 and dims[1][0] == dims[2][0] == 1
        assert P.level_state(n0, 1, faces, per)[1][0] == 0 and P.level_state(n0, 1, faces, per)[0][:2] == (1, 1)


SYM_BOXES = [(33, 47, 61), (34, 34, 34), (9, 7, 12), (4, 40, 40)]


@pytest.mark.parametrize("kind,omg", KINDS, ids=[f"{k}_{w}" for k, w in KINDS])
@pytest.mark.parametrize("s", list(P.STATES))
def test_preconditioner_is_symmetric(s, kind, omg):
    """test_mg_oracle's construction and tolerance: (M r1).r2 = r1.(M r2) to 1e-12 relative, FP64 -- mgrb on odd periodic extents, where the
    two seam points share a colour, included; <u, M u> keeps A's sign"""
    state = P.STATES[s]
    for gsz in SYM_BOXES:
        sz, idx, _ = TM._box(gsz)
        rng = np.random.default_rng(5)
        shape = (idx[3] - idx[2] + 1, idx[1] - idx[0] + 1, idx[5] - idx[4] + 1)
        r1, r2 = rng.standard_normal(shape), rng.standard_normal(shape)
        if state[2]:  # (the singular operator: residuals of zero mean, as the projections keep them)
            r1, r2 = r1 - r1.mean(), r2 - r2.mean()
        m1, m2 = _apply(kind, state, sz, idx, r1, omg), _apply(kind, state, sz, idx, r2, omg)
        a, b = float(np.vdot(m1, r2)), float(np.vdot(r1, m2))
        print(f"symmetry {s} {kind} {omg} {gsz}: {abs(a - b) / max(abs(a), abs(b)):.2e}")
        assert abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (gsz, a, b)
        assert float(np.vdot(m1, r1)) < 0.0, gsz


def _smallest_ritz(state, kind, omg, gsz=(33, 47, 61), steps=24):
    """test_mg_oracle._smallest_ritz with A the operator of the state (the oracle's residual kernel on the filled field) and M this file's
    cycle; a singular state: on the complement of the constants (every vector loses its mean, as the projections do)"""
    k = P.kernels("f64", state[0], state[1])
    sz, idx, n0 = TM._box(gsz)
    ins = M.inner(sz, idx)
    shape = (n0[1], n0[0], n0[2])
    cf = np.array(CF, dtype=np.float64)
    proj = (lambda v: v - v.mean()) if state[2] else (lambda v: v)

    def B(v):  # -A v
        x, r = k.alloc(sz), k.alloc(sz)
        x[ins] = v
        k.blas_calc_rk(r, x, k.alloc(sz), sz, idx, cf)
        return r[ins].copy()

    T = lambda v: proj(-_apply(kind, state, sz, idx, B(v), omg))  # noqa: E731
    v = proj(np.random.default_rng(9).standard_normal(shape))
    V = [v / np.sqrt(np.vdot(v, B(v)))]
    alphas, betas = [], []
    for j in range(steps):
        w = T(V[j])
        alphas.append(float(np.vdot(B(w), V[j])))
        for q in V:
            w = w - float(np.vdot(B(q), w)) * q
        beta = float(np.sqrt(max(np.vdot(w, B(w)), 0.0)))
        if beta < 1e-12 or j == steps - 1:
            break
        betas.append(beta)
        V.append(w / beta)
    n = len(alphas)
    Tm = np.diag(alphas) + np.diag(betas[: n - 1], 1) + np.diag(betas[: n - 1], -1)
    return float(np.linalg.eigvalsh(Tm).min())




@pytest.mark.parametrize("kind,omg", KINDS, ids=[f"{k}_{w}" for k, w in KINDS])
@pytest.mark.parametrize("s", list(P.STATES))
def test_preconditioned_operator_is_definite(s, kind, omg):
    lo = _smallest_ritz(P.STATES[s], kind, omg)
    print(f"smallest Ritz value of M A, {s}, {kind}, omega {omg}: {lo:.4f}")
    assert lo > 0.1, (s, kind, omg, lo)


def test_oracle_iteration_counts():
    """PCG on the seeded problem (33 x 47 x 61, FP64, exact dots, eps 1e-5; the singular states on the incompatible b, projected): the counts
    tests/test_gpu_periodic.py expects of the GPU.  mg and mgrb under periodic X and periodic X + Z stay within 1.5 x their Dirichlet counts
    (the prototype's worst ratio on this box was 7 / 6; a lost seam link shows at jacobi's level, 40 or more)"""
    b, p = PP.problem(P.COUNT_BOX, "f64", 0)
    got = {}
    for s, state in P.COUNT_STATES.items():
        for pc, coef in P.COUNT_RUNS:
            r = P.run(P.COUNT_BOX, pc, coef, "f64", state, 300, b, p, eps=1e-5)
            assert r.res < 1e-5 and len(r.history) == r.itr
            got[s, pc, coef] = r.itr
    print("iteration counts", got)
    assert got == P.COUNTS, got
    for s in ("px", "pxz"):
        for pc, coef in P.COUNT_RUNS:
            if pc in ("mg", "mgrb"):
                assert got[s, pc, coef] <= 1.5 * N.COUNTS["none", pc, coef], (s, pc, coef, got[s, pc, coef], N.COUNTS["none", pc, coef])


@pytest.mark.parametrize("c", P.PCG_CASES, ids=[c["id"] for c in P.PCG_CASES])
def test_pcg_parity_premise(c):
    """the GPU cases: FP32 no dot of the K iterations within its summation bound of a rounding boundary (and the runs with every dot at
    either edge give the same bytes); FP64 an envelope that says something"""
    state = P.STATES[c["state"]]
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    if c["prec"] == "f32":
        r0 = P.premise_f32(c["gsz"], c["pc"], c["coef"], state, c["K"], b, p, eps=1e-30)
        for q in (-1, 1):
            rq = P.case_run(c, perturb=q)
            assert rq.itr == r0.itr and rq.history == r0.history and rq.P.tobytes() == r0.P.tobytes(), (c["id"], q)
    else:
        r0, E, Eh = P.envelope_f64(c["gsz"], c["pc"], c["coef"], state, c["K"], b, p, eps=1e-30)
        h0 = np.array([v for _, v in r0.history])
        rel = max(float(E.max() / np.abs(r0.P).max()), float((Eh / h0).max()))
        assert rel <= CP.ENVELOPE_MAX, (c["id"], rel)
    assert r0.itr == c["K"]


@pytest.mark.parametrize("c,div,state", P.DECOMP, ids=[d[0]["id"] for d in P.DECOMP])
def test_decomposed_case_premise(c, div, state):
    """the decomposed GPU cases cut no periodic direction and solve to convergence before ItrMax; FP32: no dot within its summation bound of a
    rounding boundary, FP64: an envelope that says something"""
    assert all(div[d] == 1 for d in range(3) if state[1][d])
    b, p = PP.problem(c["gsz"], c["prec"], 0)
    if c["prec"] == "f32":
        r0 = P.run(c["gsz"], c["pc"], c["coef"], "f32", state, 100, b, p)
        assert not CP.flips(r0, "f32"), CP.flips(r0, "f32")[:4]
    else:
        r0, E, Eh = P.envelope_f64(c["gsz"], c["pc"], c["coef"], state, 100, b, p)
        h0 = np.array([v for _, v in r0.history])
        assert max(float(E.max() / np.abs(r0.P).max()), float((Eh / h0).max())) <= CP.ENVELOPE_MAX
    assert r0.res < O.EPS and r0.itr < 100


def test_manufactured_field_is_periodic_and_solved():
    """the manufactured problem of the GPU test: u repeats with the inner extent in the flagged directions, and the restated solve finds it"""
    gsz, faces, per = (18, 14, 20), (0, 0, 0, 1, 0, 0), P.PXZ
    u, b, p = P.manufactured(gsz, faces, per)
    assert np.array_equal(u[0, 1:-1, 1:-1], u[-2, 1:-1, 1:-1]) and np.array_equal(u[1:-1, 1:-1, -1], u[1:-1, 1:-1, 1])
    assert np.array_equal(u[1:-1, -1, 1:-1], u[1:-1, -2, 1:-1])
    r = P.run(gsz, "mgrb", 1.0, "f64", (faces, per, False), 100, b, p, eps=1e-10)
    assert 0 < r.itr < 100 and np.abs(PP.unpad(r.P) - u).max() < 1e-8


# ---- the brick-wise cycle of tests/test_mg_decomp_oracle.py with a periodic direction that the decomposition does not cut
class Bricks(TD.Bricks):
    """a brick holds the whole of an uncut direction, so its ghosts there are the wrap of the level's own array, at every distributed level (a
    level of one point: zeros); the weights come through mg_parity.weights (periodic_parity.levels)"""

    def __init__(self, gsz, div, omg, G, faces, per):
        super().__init__(gsz, div, omg, G)
        self.faces, self.per = faces, per

    def _wrapped(self, f, lev, *a):
        keep = TD._ghosted
        wrap = P.level_state(self.n0, lev, self.faces, self.per)[1]

        def ghosted(glob, sl, fill=0.0):
            if fill != fill:  # (the exchanged residual, NaN outside: not a field)
                return keep(glob, sl, fill)
            Pd = np.pad(glob, 1, constant_values=fill)
            for d in range(3):
                if wrap[d]:
                    q = np.moveaxis(Pd, P._AXIS[d], 0)
                    q[0], q[-1] = q[-2].copy(), q[1].copy()
            return Pd[tuple(slice(s.start, s.stop + 2) for s in sl)].copy()

        TD._ghosted = ghosted
        try:
            return f(*a)
        finally:
            TD._ghosted = keep

    def smooth(self, xs, bs, lev):
        return self._wrapped(super().smooth, lev, xs, bs, lev)

    def restrict(self, xs, bs, lev):
        return self._wrapped(super().restrict, lev, xs, bs, lev)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", [(32, 36, 40), (33, 47, 61)], ids=["32x36x40", "33x47x61"])
def test_brickwise_cycle_with_periodic_y_equals_single_domain(gsz, prec):
    """division (2, 1, 2), periodic Y, every allowed gather level: the brick-wise `mg` cycle assembled = the single-domain restatement, bit for
    bit"""
    div, faces, per = (2, 1, 2), N.NONE, P.PY
    k = P.kernels(prec, faces, per)
    sz, idx, n0 = TM._box(gsz)
    ins = M.inner(sz, idx)
    r = k.alloc(sz)
    r[ins] = np.random.default_rng(5).standard_normal(r[ins].shape).astype(k.real)
    ref = P.apply("mg", k, r, sz, idx, 0.8)[ins]
    Gmax = D.mg_gather_level(gsz, div, gather_points=0)
    for G in range(1, Gmax + 1):
        B = Bricks(gsz, div, k.real(0.8), G, faces, per)
        bs = [r[ins][TD._own_sl(h, m, 0)] for h, m in B.bricks]
        with P.levels(faces, per):
            got = B.assemble(B.cycle(bs, 0), 0, k.real)
        assert got.tobytes() == ref.tobytes(), f"G = {G}: the brick-wise cycle differs"
