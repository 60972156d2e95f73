"""The zebra line smoother along Z of pcg ... mgrb (cz_set_mg_lines), restated in numpy on the oracle (importable without a GPU; DESIGN.md
§5.22): what tests/test_lines_oracle.py checks on the CPU and tests/test_gpu_lines.py compares the GPU driver with.

The levels, the weights, the walk, the restriction and the prolongation are those of coefmg_parity.  Only the smoother of `mgrb` changes:
every pair of the walk runs two zebra line iterations.  The colour of row (I, J) is (I + J) & 1; a forward iteration sweeps colour 0 then
colour 1, a backward one (post) colour 1 then colour 0.  One sweep of colour c solves every row of that colour exactly along K and relaxes:

    f_K = b_K - (((X(I) u(I+1) + X(I-1) u(I-1)) + Y(J) u(J+1)) + Y(J-1) u(J-1))     (left to right, all at K)
    a_K = Z(K-1)    c_K = Z(K)    d_K = -D_K
    end K = 0   : folded ?  d_0 = d_0 + Z(-1)          :  f_0 = f_0 - Z(-1) u(-1)
    end K = n-1 : folded ?  d_{n-1} = d_{n-1} + Z(n-1) :  f_{n-1} = f_{n-1} - Z(n-1) u(n)
    forward :  cp_0 = c_0 / d_0,  dp_0 = f_0 / d_0;   m = d_K - a_K cp_{K-1},  cp_K = c_K / m,  dp_K = (f_K - a_K dp_{K-1}) / m
    backward:  y_{n-1} = dp_{n-1};   y_K = dp_K - cp_K y_{K+1}
    update  :  x_K = u_K + (y_K - u_K) omega

every operation rounded once in the precision of the arrays.  An end is folded only at level 0 on a zero-flux Z face while Z is not periodic
(the level's `mirrors`); every other end reads the ghost as the fills left it, so a periodic Z is a lagged wrap.  cp_{n-1} is not formed.
A level with ni = nj = 1 keeps the point colour sweeps of coefmg_parity.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cg_parity as CP  # noqa: E402
import coef_parity as K  # noqa: E402
import coefmg_parity as G  # noqa: E402
import mg_parity as M  # noqa: E402
import periodic_parity as P  # noqa: E402
import problem_parity as PP  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

PCG_STATES = K.PCG_STATES
STATES = K.STATES


# ---- the fields
def stretch(gsz, prec, ratio):
    """a grid refined towards both Z walls: over the brick's Z cells k = 0 .. n - 1 the cell height is h_k = ratio ** (t_k - 1) with
    t_k = min(k, n - 1 - k) / (n / 2); bx = by = h_k at cell k, bz(k) = 2 / (h_k + h_{k+1}) with h_n := h_0"""
    R = K._real(prec)
    n = gsz[2]
    k = np.arange(n)
    h = float(ratio) ** (np.minimum(k, n - 1 - k) / (n / 2.0) - 1.0)
    bz = 2.0 / (h + np.roll(h, -1))
    return [np.ascontiguousarray(np.broadcast_to(v.astype(R), tuple(gsz))) for v in (h, h, bz)]


def anisoz(gsz, prec, ratio):
    """constant by direction: bx = by = 1, bz = ratio"""
    R = K._real(prec)
    return [np.full(tuple(gsz), v, dtype=R) for v in (1.0, 1.0, float(ratio))]


FIELDS = dict(K.FIELDS)
FIELDS.update({"stretch30": lambda g, q: stretch(g, q, 30), "anisoz100": lambda g, q: anisoz(g, q, 100), "anisoz1000": lambda g, q: anisoz(g, q, 1000)})


# ---- the smoother
def row_colour(shape):
    """(I + J) & 1 of every point, arrays [j, i, k]"""
    nj, ni, nk = shape
    c = (np.arange(nj)[:, None] + np.arange(ni)[None, :]) & 1
    return np.broadcast_to(c[:, :, None], shape)


def has_lines(L):
    nj, ni, _ = L.shape
    return ni * nj > 1


def folded(L):
    """the two ends of a row that are folded: the level's mirrored Z faces (level 0 only; none while Z is periodic)"""
    return bool(L.mirrors[4]), bool(L.mirrors[5])


def line_system(u, b, L, mode=0):
    """(f, d) of every row of the level after the ends.  mode 0: from the iterate u; 1: every u a literal +0 (b, D, Z only); 2: the row's own
    values and its Z ghosts literal zeros, the other rows read from u"""
    R = b.dtype.type
    X, Y, Z = L.W
    c = slice(1, -1)
    if mode == 1:
        f = b.copy()
        p = None
    else:
        p = G.padded(u, L)
        f = b - (((X[:, 1:, :] * p[c, 2:, c] + X[:, :-1, :] * p[c, :-2, c]) + Y[1:] * p[2:, c, c]) + Y[:-1] * p[:-2, c, c])
    d = -L.D
    lo, hi = folded(L)
    n = b.shape[2]
    if lo:
        d[:, :, 0] = d[:, :, 0] + Z[:, :, 0]
    elif mode == 0:
        f[:, :, 0] = f[:, :, 0] - Z[:, :, 0] * p[c, c, 0]
    if hi:
        d[:, :, n - 1] = d[:, :, n - 1] + Z[:, :, n]
    elif mode == 0:
        f[:, :, n - 1] = f[:, :, n - 1] - Z[:, :, n] * p[c, c, n + 1]
    assert f.dtype == R and d.dtype == R
    return f, d


def thomas(f, d, Z):
    """y of every row: a_K = Z(K-1), c_K = Z(K) (Z has n + 1 entries along k, entry K + 1 the link between K and K + 1)"""
    n = f.shape[2]
    cp, dp, y = np.empty_like(f), np.empty_like(f), np.empty_like(f)
    dp[:, :, 0] = f[:, :, 0] / d[:, :, 0]
    if n > 1:
        cp[:, :, 0] = Z[:, :, 1] / d[:, :, 0]
    for k in range(1, n):
        a = Z[:, :, k]
        m = d[:, :, k] - a * cp[:, :, k - 1]
        if k < n - 1:
            cp[:, :, k] = Z[:, :, k + 1] / m
        dp[:, :, k] = (f[:, :, k] - a * dp[:, :, k - 1]) / m
    y[:, :, n - 1] = dp[:, :, n - 1]
    for k in range(n - 2, -1, -1):
        y[:, :, k] = dp[:, :, k] - cp[:, :, k] * y[:, :, k + 1]
    return y


def line_sweep(u, b, L, omg, c, mode=0):
    """one sweep of colour c in place: every row of that colour solved along K from the array as it is before the sweep, and relaxed"""
    R = b.dtype.type
    if u is None:
        u = np.zeros_like(b)
    f, d = line_system(u, b, L, mode)
    y = thomas(f, d, L.W[2])
    own = np.zeros_like(b) if mode else u
    x = own + (y - own) * R(omg)
    return np.where(row_colour(b.shape) == c, x, u)


def pair(x, b, L, omg, post):
    """two zebra line iterations (x None: from zero), forward (colour 0, 1) or backward (post); a level without X / Y links keeps the point
    colour sweeps"""
    if not has_lines(L):
        return G.pair(x, b, L, omg, "mgrb", post)
    first = 1 if post else 0
    for _ in range(2):
        x = line_sweep(line_sweep(x, b, L, omg, first), b, L, omg, 1 - first)
    return x


def pair_from_zero_forms(b, L, omg, post):
    """the first iteration of a pair from zero through the from-zero forms (modes 1 and 2), as a level that is not filled runs it"""
    first = 1 if post else 0
    x = line_sweep(None, b, L, omg, first, mode=1)
    return line_sweep(x, b, L, omg, 1 - first, mode=2)


def vcycle(b, l, H, omg):
    """x = V_l(b): mg_walk's order, no tail"""
    if l == len(H) - 1:
        x = pair(None, b, H[l], omg, False)
        x = pair(x, b, H[l], omg, False)
        for _ in range(2):
            x = pair(x, b, H[l], omg, True)
        return x
    x = pair(None, b, H[l], omg, False)
    xc = vcycle(G.restrict(x, b, H[l]), l + 1, H, omg)
    return pair(M.prolong(x, xc), b, H[l], omg, True)


def apply(H, r, sz, idx, omg):
    """z = M^-1 r of the line cycle on full S3D arrays (the cells outside the inner box stay zero)"""
    R = r.dtype.type
    ins = M.inner(sz, idx)
    z = np.zeros_like(r)
    z[ins] = vcycle(np.ascontiguousarray(r[ins]), 0, H, R(omg))
    return z


class CZ(G.CZ):
    """coefmg_parity.CZ whose mgrb cycle is the line cycle while `lines` is set and the coefficient hierarchy H is in force"""
    lines = False

    def Preconditioner(self, xx, bb, pc):
        if not (self.lines and self.H is not None and self._mgrb):
            return super().Preconditioner(xx, bb, pc)
        xx[...] = apply(self.H, bb, self.size, self.idx, self.ac1)
        self.cycles += 1


def solver(gsz, coef, prec, state, beta, perturb=0, lines=True):
    faces, per, closed = state
    assert P.solvable(faces, per, closed)
    k = K.Kernels("oracle", prec)
    k.faces, k.per = tuple(faces), tuple(per)
    cz = CZ(k, wide=False, dots="exact", perturb=perturb)
    cz.closed = bool(closed)
    cz.setup(list(gsz), coef)
    k.user = True
    k.B = K.imported(beta, per)
    cz.s = K.scaling(k.B, cz.size, cz.idx)
    cz.H = G.hierarchy(beta, gsz, state)
    cz.lines = bool(lines)
    return cz, k


def run(gsz, pc, coef, prec, state, itr_max, b, p, beta, eps=None, perturb=0, lines=True):
    """coefmg_parity.run with the line cycle as the preconditioner of mgrb (lines=False: that run itself)"""
    import closed_parity as C
    cz, k = solver(gsz, coef, prec, state, beta, perturb, lines)
    cz.P, cz.RHS = PP.pad(p), PP.pad(b)
    closed = state[2]
    mb, tol_b = C.project(cz.RHS, cz.size, cz.idx, perturb, tol=True) if closed else (None, None)
    k.mirror(cz.P, cz.size, cz.idx)
    if eps is not None:
        cz.eps = eps
    cz.cycles = 0
    itr, res = cz.PCG(cz.P, cz.RHS, itr_max, pc)
    k.mirror(cz.P, cz.size, cz.idx)
    out = O.Result(itr=itr, res=res, history=cz.history, P=cz.P, dot_log=cz.dot_log)
    out.cycles = cz.cycles
    if closed:
        out.means = [mb] + cz.means[1:]
        out.mean_tol = [tol_b, None, cz.tol_x]
        out.sum_log = cz.sum_log
        out.B = cz.RHS
    return out


def envelope_f64(gsz, pc, coef, state, itr_max, b, p, beta, eps=None):
    """FP64: the unperturbed run and the envelope of the runs with every dot (and sum) at either edge of its summation bound"""
    r = {q: run(gsz, pc, coef, "f64", state, itr_max, b, p, beta, eps=eps, perturb=q) for q in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr, [r[q].itr for q in (-1, 0, 1)]
    P0, h0 = r[0].P, np.array([v for _, v in r[0].history])
    E = np.maximum(np.abs(r[1].P - P0), np.abs(r[-1].P - P0))
    Eh = np.maximum(np.abs(np.array([v for _, v in r[1].history]) - h0), np.abs(np.array([v for _, v in r[-1].history]) - h0))
    return r[0], E, Eh


def premise_f32(gsz, pc, coef, state, itr_max, b, p, beta, eps=None):
    """the unperturbed FP32 run, after asserting that no dot lies within its summation bound of a rounding boundary and, in the closed mode,
    that the runs with every sum at either edge give its bits (coefmg_parity.premise_f32)"""
    r0 = run(gsz, pc, coef, "f32", state, itr_max, b, p, beta, eps=eps)
    f = CP.flips(r0, "f32")
    assert not f, f"dots within their summation bound of a float boundary {f[:4]}"
    if state[2]:
        for q in (-1, 1):
            rq = run(gsz, pc, coef, "f32", state, itr_max, b, p, beta, eps=eps, perturb=q)
            assert rq.itr == r0.itr and rq.history == r0.history, q
            assert rq.P.tobytes() == r0.P.tobytes() and rq.B.tobytes() == r0.B.tobytes(), q
    return r0


def inverse(H, gsz, omg):
    """M^-1 of the line cycle as a dense matrix in double on the inner cells of a small box, C order [i, j, k]: column q = M^-1 e_q"""
    sz, idx = K.box(gsz)
    n = [v - 2 for v in gsz]
    nn = n[0] * n[1] * n[2]
    Mi = np.zeros((nn, nn))
    for q in range(nn):
        e = np.zeros(tuple(gsz))
        e[1 + q // (n[1] * n[2]), 1 + (q // n[2]) % n[1], 1 + q % n[2]] = 1.0
        Mi[:, q] = PP.unpad(apply(H, PP.pad(e), sz, idx, omg))[1:-1, 1:-1, 1:-1].ravel()
    return Mi


# ---- the GPU cases (tests/test_gpu_lines.py), chosen on the CPU (tests/test_lines_oracle.py: the FP32 premise, the FP64 envelope)
def case(gsz, coef, prec, Kit, state, field, seed=0):
    return dict(gsz=tuple(gsz), pc="mgrb", coef=coef, prec=prec, K=Kit, state=state, field=field, seed=seed,
                id=f"pcg_lines_{'x'.join(map(str, gsz))}_{prec}_{state}_{field}_K{Kit}")


PCG_CASES = [
    case((9, 7, 12), 1.0, "f32", 3, "inflow", "stretch30"),
    case((9, 7, 12), 1.0, "f64", 3, "closed", "random"),
    case((33, 47, 61), 1.0, "f32", 3, "channel", "stretch30"),
    case((33, 47, 61), 0.9, "f64", 3, "dirichlet", "random"),
    case((33, 47, 61), 1.0, "f32", 3, "closed", "random"),
    case((33, 47, 61), 1.0, "f64", 3, "inflow", "stretch30"),
]


def case_problem(c):
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    return b, p, FIELDS[c["field"]](c["gsz"], c["prec"])


def case_run(c, perturb=0):
    b, p, beta = case_problem(c)
    return run(c["gsz"], c["pc"], c["coef"], c["prec"], STATES[c["state"]], c["K"], b, p, beta, eps=1e-30, perturb=perturb)


# ---- iterations to COUNT_EPS on the seeded problem at COUNT_BOX, FP64, ItrMax 300 (tests/lines_measured.py; tests/test_lines_oracle.py
# re-measures them): lines at coef 1.0 against the point colour sweeps at coef 1.2, both with the coefficient hierarchy
COUNT_BOX, COUNT_EPS = K.COUNT_BOX, K.COUNT_EPS
COUNT_FIELDS = ("anisoz100", "stretch30", "random")
COUNT_STATES = ("dirichlet", "inflow", "closed")


def count(field, state, lines):
    g = COUNT_BOX
    b, p = PP.problem(g, "f64", 0)
    return run(list(g), "mgrb", 1.0 if lines else 1.2, "f64", STATES[state], 300, b, p, FIELDS[field](g, "f64"), eps=COUNT_EPS, lines=lines).itr
