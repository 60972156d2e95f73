"""The closed box for pcg on the CPU (tests/closed_parity.py): with the mode off the restatement is neumann_parity's byte
for byte; the assembled six-face operator is symmetric with zero row sums and is what the mirrored kernels state; the masked diagonal
stays positive on every level; the V-cycles stay symmetric and, on the zero-mean subspace, definite preconditioners; the projected loop
converges on an incompatible right-hand side where the unprojected one does not; and the GPU cases of tests/test_gpu_closed.py satisfy
the premises of their bars."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cg_parity as CP  # noqa: E402
import closed_parity as CB  # noqa: E402
import mg_parity as M  # noqa: E402
import neumann_parity as N  # noqa: E402
import problem_parity as PP  # noqa: E402
import test_mg_oracle as TM  # noqa: E402
import test_neumann_oracle as TN  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

KINDS = TN.KINDS
CF = TN.CF


@pytest.mark.parametrize("pc,coef,prec", [("jacobi", 0.8, "f32"), ("mgrb", 1.2, "f64")])
def test_mode_off_is_the_neumann_restatement(pc, coef, prec):
    """five faces, closed off: the bytes, history and dots of neumann_parity.run"""
    gsz = (9, 7, 12)
    b, p = PP.problem(gsz, prec, 0)
    want = N.run(gsz, pc, coef, prec, N.FIVE, 5, b, p, eps=1e-30)
    got = CB.run(gsz, pc, coef, prec, 5, b, p, eps=1e-30, closed=False, faces=N.FIVE)
    assert got.itr == want.itr and got.history == want.history and got.P.tobytes() == want.P.tobytes() and got.dot_log == want.dot_log


def test_six_face_operator_is_symmetric_with_zero_row_sums_and_is_what_the_kernels_state():
    gsz = (9, 7, 12)  # 7 x 5 x 10 inner cells
    A = N.assembled(gsz, CB.SIX)
    assert np.abs(A - A.T).max() == 0.0 and np.abs(A.sum(axis=1)).max() == 0.0
    ev = np.linalg.eigvalsh(A)
    assert ev.max() <= 64 * np.finfo(np.float64).eps * 12 and ev[-2] < -1e-3  # one zero eigenvalue: the constants
    k = TN._kernels("f64", CB.SIX)
    sz, idx, _ = TM._box(gsz)
    ins = M.inner(sz, idx)
    u, au, r, b = (k.alloc(sz) for _ in range(4))
    u[ins] = np.random.default_rng(2).standard_normal(u[ins].shape)
    k.blas_calc_ax(au, u, sz, idx, np.array(CF, dtype=np.float64))
    v = PP.unpad(u)[1:-1, 1:-1, 1:-1].ravel()
    tol = 64 * np.finfo(np.float64).eps * np.abs(v).max()
    assert np.abs(PP.unpad(au)[1:-1, 1:-1, 1:-1].ravel() - A @ v).max() <= tol
    k.blas_calc_rk(r, u, b, sz, idx, np.array(CF, dtype=np.float64))
    assert np.abs(PP.unpad(r)[1:-1, 1:-1, 1:-1].ravel() + A @ v).max() <= tol


@pytest.mark.parametrize("gsz", CB.BOXES + [(512, 512, 512), (6, 6, 6), (5, 4, 3)], ids=lambda g: "x".join(map(str, g)))
def test_masked_diagonal_is_positive_on_every_level(gsz):
    """D = Wx cx + Wy cy + Wz cz with six faces: zero only at a point that is first and last in all three directions, which no level of a
    hierarchy has -- coarsening stops at the first level whose largest extent is <= 4, so the coarsest has >= 3 points along its longest
    direction (ceil(n / 2) >= 3 for n >= 5); a level-0 box of <= 4 everywhere is its own coarsest level and keeps level 0's D = 6"""
    n0 = tuple(v - 2 for v in gsz)
    dims = M.level_dims(n0)
    if len(dims) > 1:
        assert max(dims[-1]) >= 3
    for level, (ni, nj, nk) in enumerate(dims):
        if level == 0:
            continue
        cx, cy, cz = N.links(ni, 1, 1), N.links(nj, 1, 1), N.links(nk, 1, 1)
        ex, ey, ez = M.extents(n0[0], level, ni), M.extents(n0[1], level, nj), M.extents(n0[2], level, nk)
        # min over the level of D: every term is a product of positive extents and a link count, so the minimum is reached on the corners
        d = (ey[:, None, None] * ez[None, None, :] * cx[None, :, None] + ex[None, :, None] * ez[None, None, :] * cy[:, None, None]
             + ey[:, None, None] * ex[None, :, None] * cz[None, None, :]) if ni * nj * nk <= 1 << 22 else None
        if d is None:  # (512^3: the corner values bound the level)
            corner = [ey[j] * ez[k] * cx[i] + ex[i] * ez[k] * cy[j] + ey[j] * ex[i] * cz[k] for i in (0, -1) for j in (0, -1) for k in (0, -1)]
            assert min(corner) > 0, (level, corner)
        else:
            assert (d > 0).all(), level
            if ni * nj * nk <= 1 << 16:
                assert (N.weights(n0, level, np.float64, CB.SIX)[3] == d).all()


@pytest.mark.parametrize("kind,omg", KINDS, ids=[f"{k}_{w}" for k, w in KINDS])
def test_preconditioner_is_symmetric(kind, omg):
    """test_mg_oracle's construction and tolerance with six faces: (M r1).r2 = r1.(M r2) to 1e-12 relative, FP64"""
    for gsz in ((33, 47, 61), (9, 7, 12), (3, 40, 40)):
        sz, idx, _ = TM._box(gsz)
        rng = np.random.default_rng(5)
        shape = (idx[3] - idx[2] + 1, idx[1] - idx[0] + 1, idx[5] - idx[4] + 1)
        r1, r2 = rng.standard_normal(shape), rng.standard_normal(shape)
        a = float(np.vdot(TN._apply(kind, CB.SIX, sz, idx, r1, omg), r2))
        b = float(np.vdot(r1, TN._apply(kind, CB.SIX, sz, idx, r2, omg)))
        assert abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (gsz, a, b)


def _lanczos_zero_mean(kind, omg, gsz, steps=24):
    """test_mg_oracle._smallest_ritz on the zero-mean subspace: Lanczos on M N in the inner product of B = -N with full
    re-orthogonalisation.  B is semi-definite, its null space the constants, so it is an inner product on the zero-mean fields: the start
    vector and every new vector are projected there (the constant M N v may carry has no B-norm and B never sees it)"""
    sz, idx, n0 = TM._box(gsz)
    shape = (n0[1], n0[0], n0[2])
    k = TN._kernels("f64", CB.SIX)
    ins = M.inner(sz, idx)

    def B(v):  # -N v through the mirrored kernel
        u, au = k.alloc(sz), k.alloc(sz)
        u[ins] = v
        k.blas_calc_ax(au, u, sz, idx, np.array(CF, dtype=np.float64))
        return -au[ins]

    def T(v):  # M N v, zero mean
        w = -TN._apply(kind, CB.SIX, sz, idx, B(v), omg)
        return w - w.mean()

    v = np.random.default_rng(9).standard_normal(shape)
    v -= v.mean()
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
def test_preconditioned_operator_is_definite_on_the_zero_mean_subspace(kind, omg):
    lo = _lanczos_zero_mean(kind, omg, (33, 47, 61))
    print(f"smallest Ritz value of M N on the zero-mean subspace, six faces, {kind}, omega {omg}: {lo:.4f}")
    assert lo > 0.0, (kind, omg, lo)


@pytest.fixture(scope="module")
def seeded():
    return PP.problem(CB.COUNT_BOX, "f64", 0)


def test_iteration_counts_and_the_mean_of_the_answer(seeded):
    """33 x 47 x 61, FP64, eps 1e-5, ItrMax 300, the seeded b (mean -1.0e-5: incompatible): the projected loop converges in the counts
    tests/test_gpu_closed.py expects of the GPU, and the mean of every answer is within closed_parity.mean_bound"""
    b, p = seeded
    got, mx = {}, {}
    for pc, coef in CB.COUNT_RUNS:
        r = CB.run(CB.COUNT_BOX, pc, coef, "f64", 300, b, p, eps=1e-5)
        assert r.res < 1e-5 and len(r.history) == r.itr < 300
        got[pc, coef] = r.itr
        x = PP.unpad(r.P)[1:-1, 1:-1, 1:-1]
        mean = math.fsum(x.ravel()) / x.size
        bound = CB.mean_bound(r.means[2], np.abs(x).max(), np.float64)
        print(f"closed {pc} {coef}: {r.itr} iterations, means {[float(v) for v in r.means]}, mean of the answer {mean:.3e} (bound {bound:.3e})")
        assert abs(mean) <= bound, (pc, mean, bound)
        assert abs(float(r.means[0]) - (-1.0e-5)) < 2e-6
        mx[pc] = (mean, bound)
    assert got == CB.COUNTS, got
    # the same field whichever preconditioner ran: two answers differ by their iteration errors (res < 1e-5), not by an offset -- the means
    # of any two lie within the sum of the two runs' own bounds of each other
    for pc in ("jacobi", "mg", "mgrb"):
        assert abs(mx[pc][0] - mx["none"][0]) <= mx[pc][1] + mx["none"][1], (pc, mx[pc], mx["none"])


def test_the_unprojected_loop_does_not_converge_on_the_incompatible_b(seeded):
    """neumann_parity's loop (closed off) with six faces on the same problem: `none` has not converged after 300 iterations and the mean of
    its iterate has run away"""
    b, p = seeded
    r = CB.run(CB.COUNT_BOX, "none", 0.8, "f64", 300, b, p, eps=1e-5, closed=False)
    assert r.itr == 300 and not (r.res < 1e-5), (r.itr, r.res)


@pytest.mark.parametrize("c", CB.CASES, ids=[c["id"] for c in CB.CASES])
def test_pcg_parity_premise(c):
    """the GPU cases: FP32 no dot within its bound of a rounding boundary and the runs with every dot and sum at either edge give the same
    bytes; FP64 an envelope that says something; every box within the depth the bound of the sums assumes"""
    assert CB.depth(c["gsz"], c["prec"]) <= CB.SUM_DEPTH
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    if c["prec"] == "f32":
        r0 = CB.premise_f32(c["gsz"], c["pc"], c["coef"], c["K"], b, p, eps=1e-30)
    else:
        r0, E, Eh = CB.envelope_f64(c["gsz"], c["pc"], c["coef"], c["K"], b, p, eps=1e-30)
        h0 = np.array([v for _, v in r0.history])
        rel = max(float(E.max() / np.abs(r0.P).max()), float((Eh / h0).max()))
        assert rel <= CP.ENVELOPE_MAX, (c["id"], rel)
    assert r0.itr == c["K"]


@pytest.mark.parametrize("c,div", CB.DECOMP, ids=[d[0]["id"] for d in CB.DECOMP])
def test_decomposed_case_premise_and_brickwise_sums(c, div):
    """the decomposed GPU cases converge within ItrMax 100 (FP32: with the premise of bit equality through convergence); and the projection
    restated brick by brick -- every brick's correctly rounded sum, the sums of the bricks added correctly rounded, one mean for all -- is
    the single-domain projection byte for byte"""
    gsz, prec = c["gsz"], c["prec"]
    assert CB.depth(gsz, prec) <= CB.SUM_DEPTH
    b, p = PP.problem(gsz, prec, c.get("seed", 0))
    if prec == "f32":
        r = CB.premise_f32(gsz, c["pc"], c["coef"], 100, b, p)
    else:
        r = CB.run(gsz, c["pc"], c["coef"], prec, 100, b, p)
    assert r.res < O.EPS and r.itr < 100
    R = b.dtype.type
    inner = b[1:-1, 1:-1, 1:-1]
    cuts = [np.array_split(np.arange(inner.shape[d]), div[d]) for d in range(3)]
    parts = [math.fsum(inner[np.ix_(ci, cj, ck)].astype(np.float64).ravel()) for ci in cuts[0] for cj in cuts[1] for ck in cuts[2]]
    m = R(math.fsum(parts) / inner.size)
    whole = PP.pad(b)
    sz, idx, _ = TM._box(gsz)
    assert float(CB.project(whole, sz, idx)) == float(m)
    brick = b.copy()
    for ci in cuts[0]:
        for cj in cuts[1]:
            for ck in cuts[2]:
                sl = np.ix_(ci + 1, cj + 1, ck + 1)
                brick[sl] = brick[sl] - m
    assert PP.pad(brick).tobytes() == whole.tobytes()


def test_kernel_case_premise():
    """tests/test_gpu_closed.py's shift_sums_k and cg_update cases, FP32: neither sum of the shifted array within its bound of a float
    boundary (the GPU must then give the restatement's REAL)"""
    import test_gpu_closed as TG
    for gsz in TG.KERNEL_BOXES:
        a, m = TG.kernel_field(gsz, "f32")
        for shift in (False, True):
            for t in TG.shift_terms(a, m if shift else None, gsz):
                S, B = CB.sum_bound(t)
                assert np.float32(S - B) == np.float32(S + B), (gsz, shift, S, B)
