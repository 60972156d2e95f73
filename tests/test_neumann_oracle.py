"""Zero-flux (Neumann) faces for pcg on the CPU (tests/neumann_parity.py): without a mask the restatement is that of
tests/mg_parity.py and tests/mgrb_parity.py byte for byte; the mirrored kernels state the assembled zero-flux operator; the V-cycles with
the masked diagonal stay symmetric definite preconditioners; PCG converges in the iteration counts the GPU test expects; and the GPU cases
of tests/test_gpu_neumann.py satisfy the premises of their bars."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cg_parity as CP  # noqa: E402
import mg_parity as M  # noqa: E402
import mgrb_parity as RB  # noqa: E402
import neumann_parity as N  # noqa: E402
import problem_parity as PP  # noqa: E402
import test_mg_decomp_oracle as TD  # noqa: E402
import test_mg_oracle as TM  # noqa: E402
from cubez_amd import decomp as D  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

SYM_MASKS = ("z", "xp", "five")
KINDS = [("mg", 0.8), ("mgrb", 0.8), ("mgrb", 1.0), ("mgrb", 1.2)]
CF = [1, 1, 1, 1, 1, 1, 6]


def _kernels(prec, faces):
    k = N.Kernels("oracle", prec)
    k.faces = tuple(faces)
    return k


def _apply(kind, faces, sz, idx, v_inner, omg):
    k = _kernels("f64", faces)
    r = k.alloc(sz)
    ins = M.inner(sz, idx)
    r[ins] = v_inner
    return N.apply(kind, k, r, sz, idx, omg, faces)[ins]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", [(9, 7, 12), (33, 47, 61), (6, 6, 6)])
def test_no_mask_is_the_existing_restatement(gsz, prec):
    """a mask of zero: the bytes of mg_parity.apply / mgrb_parity.apply, and of their coarse cycles under `masked`"""
    k, k0 = _kernels(prec, N.NONE), O.Kernels("oracle", prec)
    sz, idx, n0 = TM._box(gsz)
    ins = M.inner(sz, idx)
    r = k.alloc(sz)
    r[ins] = np.random.default_rng(1).standard_normal(r[ins].shape).astype(k.real)
    for kind, ref, cycle in (("mg", M.apply, M.vcycle), ("mgrb", RB.apply, RB.vcycle)):
        assert N.apply(kind, k, r, sz, idx, 0.8, N.NONE).tobytes() == ref(k0, r, sz, idx, 0.8).tobytes(), kind
        plain = cycle(r[ins], 0, n0, k.real(0.8))
        with N.masked(N.NONE):
            assert cycle(r[ins], 0, n0, k.real(0.8)).tobytes() == plain.tobytes(), kind
    assert M.weights is N._UNMASKED_WEIGHTS
    assert N.restrict0(r, r, sz, idx).tobytes() == M.restrict(r[ins], r[ins], 0, n0).tobytes()


def test_the_masked_diagonal_fails_without_the_rule():
    """the feature on the CPU: with a mask the coarse diagonal is not 2 (Wx + Wy + Wz), and level 0's is"""
    n0 = (7, 5, 10)
    for level in range(len(M.level_dims(n0))):
        plain, masked = M.weights(n0, level, np.float64), N.weights(n0, level, np.float64, N.FIVE)
        for a, b in zip(plain[:3], masked[:3]):
            assert a.tobytes() == b.tobytes()
        assert (plain[3].tobytes() == masked[3].tobytes()) == (level == 0), level
    # a corner point of level 1 that lies on three Neumann faces: one link per direction
    wx, wy, wz, d = N.weights(n0, 1, np.float64, N.FIVE)
    assert d[0, 0, 0] == wx[0, 0, 0] + wy[0, 0, 0] + wz[0, 0, 0]
    # Z+ stays Dirichlet: the last point along k keeps both links
    assert d[0, 0, -1] == wx[0, 0, -1] + wy[0, 0, -1] + 2 * wz[0, 0, -1]


@pytest.mark.parametrize("mask", ["none", "z", "xp", "five", "minus3"])
def test_mirrored_calc_ax_is_the_assembled_operator(mask):
    """the oracle's blas_calc_ax on a mirrored field = N u with N assembled entry by entry (7 x 5 x 10 inner cells, zero Dirichlet values); N is
    symmetric and negative definite"""
    faces = dict(N.MASKS, minus3=N.MINUS3)[mask]
    gsz = (9, 7, 12)
    k = _kernels("f64", faces)
    sz, idx, _ = TM._box(gsz)
    ins = M.inner(sz, idx)
    u, au = k.alloc(sz), k.alloc(sz)
    u[ins] = np.random.default_rng(2).standard_normal(u[ins].shape)
    k.blas_calc_ax(au, u, sz, idx, np.array(CF, dtype=np.float64))
    A = N.assembled(gsz, faces)
    v = PP.unpad(u)[1:-1, 1:-1, 1:-1].ravel()
    got = PP.unpad(au)[1:-1, 1:-1, 1:-1].ravel()
    assert np.abs(got - A @ v).max() <= 64 * np.finfo(np.float64).eps * np.abs(v).max()  # 7 terms of size |v|, each rounded
    assert np.abs(A - A.T).max() == 0.0 and np.linalg.eigvalsh(A).max() < 0.0
    # and the residual kernel states the same operator
    r, b = k.alloc(sz), k.alloc(sz)
    k.blas_calc_rk(r, u, b, sz, idx, np.array(CF, dtype=np.float64))
    assert np.abs(PP.unpad(r)[1:-1, 1:-1, 1:-1].ravel() + A @ v).max() <= 64 * np.finfo(np.float64).eps * np.abs(v).max()


@pytest.mark.parametrize("kind,omg", KINDS, ids=[f"{k}_{w}" for k, w in KINDS])
@pytest.mark.parametrize("mask", SYM_MASKS)
def test_preconditioner_is_symmetric(mask, kind, omg):
    """test_mg_oracle's construction and tolerance: (M r1).r2 = r1.(M r2) to 1e-12 relative, FP64"""
    faces = N.MASKS[mask]
    for gsz in ((33, 47, 61), (9, 7, 12), (40, 40, 100)):
        sz, idx, _ = TM._box(gsz)
        rng = np.random.default_rng(5)
        shape = (idx[3] - idx[2] + 1, idx[1] - idx[0] + 1, idx[5] - idx[4] + 1)
        r1, r2 = rng.standard_normal(shape), rng.standard_normal(shape)
        a = float(np.vdot(_apply(kind, faces, sz, idx, r1, omg), r2))
        b = float(np.vdot(r1, _apply(kind, faces, sz, idx, r2, omg)))
        assert abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (gsz, a, b)


def _residual0(faces):
    """mg_parity.residual whose level 0 reads the mirror across the Neumann faces (inner arrays [j, i, k])"""
    keep = M.residual

    def residual(x, b, level, n0):
        if level != 0:
            return keep(x, b, level, n0)
        p = np.pad(x, 1)
        for f, (dst, src) in enumerate((((slice(None), 0), (slice(None), 1)), ((slice(None), -1), (slice(None), -2)), ((0,), (1,)), ((-1,), (-2,)),
                                        ((Ellipsis, 0), (Ellipsis, 1)), ((Ellipsis, -1), (Ellipsis, -2)))):
            if faces[f]:
                p[dst] = p[src]
        ss = p[1:-1, 2:, 1:-1] + p[1:-1, :-2, 1:-1] + p[2:, 1:-1, 1:-1] + p[:-2, 1:-1, 1:-1] + p[1:-1, 1:-1, 2:] + p[1:-1, 1:-1, :-2]
        return b - (ss - x.dtype.type(6) * x)

    return residual


@pytest.mark.parametrize("kind,omg", KINDS, ids=[f"{k}_{w}" for k, w in KINDS])
@pytest.mark.parametrize("mask", SYM_MASKS)
def test_preconditioned_operator_is_definite(mask, kind, omg, monkeypatch):
    """the smallest Ritz value of M N (test_mg_oracle's Lanczos, its A exchanged for the zero-flux operator) stays positive; printed for
    DESIGN.md §5.13"""
    faces = N.MASKS[mask]
    monkeypatch.setattr(M, "residual", _residual0(faces))
    monkeypatch.setattr(TM, "_apply", lambda k, sz, idx, v, w: _apply(kind, faces, sz, idx, v, w))
    lo = TM._smallest_ritz((33, 47, 61), omg)
    print(f"smallest Ritz value of M N, mask {mask}, {kind}, omega {omg}: {lo:.4f}")
    assert lo > 0.0, (mask, kind, omg, lo)


def test_a_level_of_one_point_between_two_neumann_faces_keeps_a_positive_diagonal():
    """(3, 40, 40) with both X faces Neumann: every level has one point in x, cx = 0 there, and D = Wy cy + Wz cz > 0"""
    sz, idx, n0 = TM._box((3, 40, 40))
    dims = M.level_dims(n0)
    assert all(d[0] == 1 for d in dims) and len(dims) > 2
    for level in range(1, len(dims)):
        wx, wy, wz, d = N.weights(n0, level, np.float64, N.X_BOTH)
        assert (d > 0).all() and (d == 2 * (wy + wz)).all(), level
    for kind, omg in KINDS:
        rng = np.random.default_rng(5)
        shape = (n0[1], n0[0], n0[2])
        r1, r2 = rng.standard_normal(shape), rng.standard_normal(shape)
        m1, m2 = _apply(kind, N.X_BOTH, sz, idx, r1, omg), _apply(kind, N.X_BOTH, sz, idx, r2, omg)
        a, b = float(np.vdot(m1, r2)), float(np.vdot(r1, m2))
        assert np.isfinite(m1).all() and abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (kind, omg, a, b)
        assert float(np.vdot(m1, r1)) < 0.0  # A's sign


def test_oracle_iteration_counts():
    """PCG on a caller's problem (33 x 47 x 61, FP64, exact dots, eps 1e-5) with no mask and with five Neumann faces: the counts
    tests/test_gpu_neumann.py expects of the GPU.  Multigrid does not notice the faces; the other preconditioners do"""
    gsz = (33, 47, 61)
    b, p = PP.problem(gsz, "f64", 0)
    got = {}
    for mask in ("none", "five"):
        for pc, coef in N.COUNT_RUNS:
            r = N.run(gsz, pc, coef, "f64", N.MASKS[mask], 1000, b, p, eps=1e-5)
            assert r.res < 1e-5 and len(r.history) == r.itr
            got[mask, pc, coef] = r.itr
    print("iteration counts", got)
    assert got == N.COUNTS, got
    for pc, coef in N.COUNT_RUNS:
        if pc in ("mg", "mgrb"):
            assert abs(got["five", pc, coef] - got["none", pc, coef]) <= 1, (pc, coef)
        else:
            assert got["five", pc, coef] > got["none", pc, coef], (pc, coef)


@pytest.mark.parametrize("c", N.PCG_CASES, ids=[c["id"] for c in N.PCG_CASES])
def test_pcg_parity_premise(c):
    """the GPU cases: FP32 no dot of the K iterations within its summation bound of a rounding boundary (and the runs with every dot at
    either edge give the same bytes); FP64 an envelope that says something"""
    if c["prec"] == "f32":
        r0 = N.case_run(c)
        f = CP.flips(r0, "f32")
        assert not f, f"{c['id']}: premise fails (choose another case): {f[:4]}"
        for q in (-1, 1):
            rq = N.case_run(c, perturb=q)
            assert rq.itr == r0.itr and rq.history == r0.history and rq.P.tobytes() == r0.P.tobytes(), (c["id"], q)
    else:
        b, p = PP.problem(c["gsz"], "f64", c["seed"])
        r0, E, Eh = N.envelope_f64(c["gsz"], c["pc"], c["coef"], c["faces"], c["K"], b, p, eps=1e-30)
        h0 = np.array([v for _, v in r0.history])
        rel = max(float(E.max() / np.abs(r0.P).max()), float((Eh / h0).max()))
        assert rel <= CP.ENVELOPE_MAX, (c["id"], rel)
    assert r0.itr == c["K"]


@pytest.mark.parametrize("c,div,faces", N.DECOMP, ids=[d[0]["id"] for d in N.DECOMP])
def test_decomposed_case_premise(c, div, faces):
    """the decomposed GPU cases solve to convergence before ItrMax; FP32: no dot within its summation bound of a rounding boundary (an
    all-reduce is one more summation order), FP64: an envelope that says something"""
    b, p = PP.problem(c["gsz"], c["prec"], 0)
    if c["prec"] == "f32":
        r0 = N.run(c["gsz"], c["pc"], c["coef"], "f32", faces, 100, b, p)
        assert not CP.flips(r0, "f32"), CP.flips(r0, "f32")[:4]
    else:
        r0, E, Eh = N.envelope_f64(c["gsz"], c["pc"], c["coef"], faces, 100, b, p)
        h0 = np.array([v for _, v in r0.history])
        assert max(float(E.max() / np.abs(r0.P).max()), float((Eh / h0).max())) <= CP.ENVELOPE_MAX
    assert r0.res < O.EPS and r0.itr < 100


# ---- the brick-wise cycle of tests/test_mg_decomp_oracle.py with a mask
class Bricks(TD.Bricks):
    """level 0's ghosts outside the box are the mirror across the Neumann faces (every brick mirrors the faces that are physical on it, which
    is the mirror of the assembled field); the levels >= 1 take the masked diagonal through mg_parity.weights (neumann_parity.masked)"""

    def __init__(self, gsz, div, omg, G, faces):
        super().__init__(gsz, div, omg, G)
        self.faces = faces

    def _mirrored(self, f, *a):
        keep, faces = TD._ghosted, self.faces

        def ghosted(glob, sl, fill=0.0):
            if fill != fill:  # (the exchanged residual, NaN outside: not a field)
                return keep(glob, sl, fill)
            P = np.pad(glob, 1, constant_values=fill)
            for q, (dst, src) in enumerate((((slice(None), 0), (slice(None), 1)), ((slice(None), -1), (slice(None), -2)), ((0,), (1,)), ((-1,), (-2,)),
                                            ((Ellipsis, 0), (Ellipsis, 1)), ((Ellipsis, -1), (Ellipsis, -2)))):
                if faces[q]:
                    P[dst] = P[src]
            return P[tuple(slice(s.start, s.stop + 2) for s in sl)].copy()

        TD._ghosted = ghosted
        try:
            return f(*a)
        finally:
            TD._ghosted = keep

    def smooth(self, xs, bs, lev):
        return self._mirrored(super().smooth, xs, bs, lev) if lev == 0 else super().smooth(xs, bs, lev)

    def restrict(self, xs, bs, lev):
        return self._mirrored(super().restrict, xs, bs, lev) if lev == 0 else super().restrict(xs, bs, lev)


BRICK_CASES = [((33, 47, 61), (2, 2, 2), "five"), ((32, 36, 40), (2, 1, 2), "five"), ((34, 30, 40), (1, 3, 1), "z"), ((40, 40, 9), (1, 1, 3), "z"),
               ((20, 21, 22), (2, 2, 2), "xp"), ((6, 6, 6), (2, 1, 1), "five")]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz,div,mask", BRICK_CASES, ids=[f"{'x'.join(map(str, g))}_{'x'.join(map(str, d))}_{m}" for g, d, m in BRICK_CASES])
def test_brickwise_cycle_with_a_mask_equals_single_domain(gsz, div, mask, prec):
    """every allowed gather level: the brick-wise `mg` cycle assembled = the single-domain restatement (level 0 through the oracle's jacobi), bit
    for bit"""
    faces = N.MASKS[mask]
    k = _kernels(prec, faces)
    sz, idx, n0 = TM._box(gsz)
    ins = M.inner(sz, idx)
    r = k.alloc(sz)
    r[ins] = np.random.default_rng(5).standard_normal(r[ins].shape).astype(k.real)
    ref = N.apply("mg", k, r, sz, idx, 0.8, faces)[ins]
    dims = D.mg_level_dims(gsz)
    Gmax = D.mg_gather_level(gsz, div, gather_points=0)
    for G in sorted({g for g in range(1, Gmax + 1)} | {Gmax}):
        if len(dims) == 1:
            G = 0
        B = Bricks(gsz, div, k.real(0.8), G, faces)
        bs = [r[ins][TD._own_sl(h, m, 0)] for h, m in B.bricks]
        with N.masked(faces):
            got = B.assemble(B.cycle(bs, 0), 0, k.real)
        assert got.tobytes() == ref.tobytes(), f"G = {G}: the brick-wise cycle differs"
