"""Periodic directions for pcg on the GPU (-m gpu), every result against the restatement of tests/periodic_parity.py: the
fill kernel alone; the V-cycles with wrapped levels (cz_precondition, byte for byte, CZ_MG_TAIL 0 and 1); PCG iteration by iteration on a
caller's problem against the exact-dot restatement; counts to convergence; the singular problems (channel, triply periodic box);
decomposed runs on the LOCAL transport; a manufactured periodic solution; mixed-precision refinement; the refusals, the state and the
invariant of the face layers."""
import ctypes as C
import math
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_parity as CB  # noqa: E402
import mg_parity as M  # noqa: E402
import neumann_parity as N  # noqa: E402
import periodic_parity as P  # noqa: E402
import problem_parity as PP  # noqa: E402
import test_gpu_neumann as TN  # noqa: E402
from cubez_amd import decomp as D  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = O.GUIDE
OMG = {"mg": 0.8, "mgrb": 1.2}


def _handle(prec, args, state=None):
    """a set-up handle under state = (faces, per, closed): the mask or the closed mode first, then the periodic directions"""
    from cubez_amd import CZ
    cz = CZ(prec, quiet=True)
    assert cz.setup(list(args)) == 1
    if state is not None:
        faces, per, closed = state
        if closed:
            cz.set_closed_box(True)
        elif any(faces):
            cz.set_neumann(faces)
        cz.set_periodic(per)
    return cz


# ---- the fill kernel alone
FILL_KINDS = {"wrap_x": [2, 2, 0, 0, 0, 0], "wrap_z": [0, 0, 0, 0, 2, 2], "wrap_y_mirror_xp": [0, 1, 2, 2, 0, 0], "wrap_xyz": [2, 2, 2, 2, 2, 2]}


def _filled(host, sz, idx, kinds):
    faces = [1 if v == 1 else 0 for v in kinds]
    per = [1 if kinds[2 * d] == 2 else 0 for d in range(3)]
    return P.fill(host.copy(), sz, idx, faces, per)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", list(FILL_KINDS))
@pytest.mark.parametrize("gsz", [(9, 7, 12), (33, 47, 61), (40, 40, 1100)], ids=["9x7x12", "33x47x61", "40x40x1100"])
def test_fill_kernel_writes_the_named_face_cells_only(gsz, name, prec):
    """czhip_fill_faces_async on an array full of random numbers: the named face cells take their source layer, every other byte (edges,
    corners, guide cells, the other faces) stays; one launch whatever the number of faces"""
    from cubez_amd.lib import CzHip
    hip = CzHip(prec)
    kinds = FILL_KINDS[name]
    sz, idx = TN._box(gsz)
    host = np.random.default_rng(31).random((gsz[1] + 2 * G, gsz[0] + 2 * G, gsz[2] + 2 * G)).astype(hip.real)
    d = hip.alloc(sz, host)
    try:
        hip.timing(True)
        assert hip.fill_faces(d, sz, idx, kinds)
        want = _filled(host, sz, idx, kinds)
        assert not np.array_equal(want, host)
        assert d.get().tobytes() == want.tobytes()
        assert hip.timing_read("bc_mirror")[0] == 1
    finally:
        hip.timing(False)
        hip.sync()
        d.free()


def test_fill_kernel_refusals():
    """half a wrap, a wrap on a face that is not physical on the brick, a kind that does not exist: refused, not a byte written; a mirror on
    a face that is not physical is skipped as czhip_mirror_faces_async skips it"""
    from cubez_amd.lib import CzHip
    hip = CzHip("f32")
    gsz = (9, 7, 12)
    sz, idx = TN._box(gsz)
    host = np.random.default_rng(32).random((gsz[1] + 2 * G, gsz[0] + 2 * G, gsz[2] + 2 * G)).astype(np.float32)
    d = hip.alloc(sz, host)
    try:
        assert not hip.fill_faces(d, sz, idx, [2, 0, 0, 0, 0, 0]) and not hip.fill_faces(d, sz, idx, [0, 0, 1, 2, 0, 0])
        assert not hip.fill_faces(d, sz, idx, [0, 0, 0, 0, 3, 0]) and not hip.fill_faces(d, sz, idx, [0, 0, 0, 0, 0, -1])
        idx_b = [1, idx[1], 2, idx[3], 2, idx[5]]  # a brick whose X- side is rank-internal
        assert not hip.fill_faces(d, sz, idx_b, [2, 2, 0, 0, 0, 0])
        idx_c = [2, sz[0], 2, idx[3], 2, idx[5]]
        assert not hip.fill_faces(d, sz, idx_c, [2, 2, 0, 0, 0, 0])
        assert d.get().tobytes() == host.tobytes()
        assert hip.fill_faces(d, sz, idx_b, [1, 1, 0, 0, 2, 2])
        assert d.get().tobytes() == P.fill(host.copy(), sz, idx_b, [1, 1, 0, 0, 0, 0], P.PZ).tobytes()
    finally:
        hip.sync()
        d.free()


# ---- the V-cycles: cz_precondition against the restatement
X_STATES = ("px", "pxz_ym", "channel", "triple")
CYCLE_CASES = [((9, 7, 12), X_STATES), ((33, 47, 61), X_STATES), ((34, 34, 34), X_STATES), ((4, 40, 40), X_STATES), ((3, 40, 40), ("pyz", "pyz_closed"))]
CYCLE_STATES = dict(P.STATES, pyz=(N.NONE, P.PYZ, False), pyz_closed=(CB.SIX, P.PYZ, True))


def _cycle_gpu(prec, gsz, kind, state):
    sz, idx, ins, r = TN._cycle_rhs(prec, gsz)
    cz = _handle(prec, list(gsz) + ["pcg", 1, OMG[kind], kind], state)
    try:
        z = cz.precondition(r)
        assert cz.precondition(r).tobytes() == z.tobytes(), "the second cycle differs"
        assert cz.info()["periodic"] == P.bits(state[1])
        return z[ins]
    finally:
        cz.close()


_TAIL0_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import numpy as np
    import test_gpu_periodic as T
    out = {{}}
    for gsz, states in T.CYCLE_CASES:
        for prec in ("f32", "f64"):
            for kind in ("mg", "mgrb"):
                for s in states:
                    out["_".join(map(str, gsz)) + prec + kind + s] = T._cycle_gpu(prec, gsz, kind, T.CYCLE_STATES[s])
    np.savez({path!r}, **out)
    """)


@pytest.fixture(scope="module")
def tail0(tmp_path_factory):
    """every cycle case with CZ_MG_TAIL=0, computed once in a child process (the variable is read when the hierarchy is created)"""
    path = str(tmp_path_factory.mktemp("periodic") / "tail0.npz")
    env = dict(os.environ, CZ_MG_TAIL="0")
    p = subprocess.run([sys.executable, "-c", _TAIL0_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return np.load(path)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz,states", CYCLE_CASES, ids=["x".join(map(str, g)) for g, _ in CYCLE_CASES])
def test_precondition_equals_the_restatement(gsz, states, prec, tail0):
    """mg and mgrb, byte for byte, the tail kernel and the level kernels giving equal bits.  (33, 47, 61): odd periodic extents, the seam points
    share a colour; (34, 34, 34): even ones; (4, 40, 40): two points in x, both links reach the same neighbour; (9, 7, 12) and (3, 40, 40):
    levels of one point in a periodic direction"""
    sz, idx, ins, r = TN._cycle_rhs(prec, gsz)
    for kind in ("mg", "mgrb"):
        for s in states:
            faces, per, closed = CYCLE_STATES[s]
            k = P.kernels(prec, faces, per)
            ref = P.apply(kind, k, r, sz, idx, OMG[kind])[ins]
            z = _cycle_gpu(prec, gsz, kind, CYCLE_STATES[s])
            assert z.tobytes() == ref.tobytes(), (kind, s)
            assert tail0["_".join(map(str, gsz)) + prec + kind + s].tobytes() == z.tobytes(), f"{kind} {s}: CZ_MG_TAIL=0 changed the bits"


# ---- PCG on a caller's problem, K iterations against the exact-dot restatement
def _pcg_gpu(c, b, p, state, itr_max, eps, division=None):
    cz = _handle(c["prec"], list(c["gsz"]) + ["pcg", itr_max, c["coef"], c["pc"]] + (list(division) if division else []))
    try:
        cz.timing(True)
        if state is not None:
            faces, per, closed = state
            if closed:
                cz.set_closed_box(True)
            elif any(faces):
                cz.set_neumann(faces)
            cz.set_periodic(per)
        cz.set_rhs(b)
        cz.set_field(p)
        cz.set_eps(eps)
        itr = cz.solve()
        return dict(itr=itr, hist=list(cz.history()), P=cz.field(), X=cz.get_field(), info=cz.info(), launches=cz.launches(),
                    means=[cz.closed_mean(w) for w in range(3)])
    finally:
        cz.timing(False)
        cz.close()


@pytest.mark.parametrize("c", P.PCG_CASES, ids=[c["id"] for c in P.PCG_CASES])
def test_pcg_iterations_vs_exact_dot_restatement(c):
    """FP32: count, history and the whole padded field bit for bit; FP64: within 2 E + 8 ulp (problem_parity.f64_close); the periodic handle
    runs fills under bc_mirror, none of the fused pairs and not the fused direction"""
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    state = P.STATES[c["state"]]
    g = _pcg_gpu(c, b, p, state, c["K"], 1e-30)
    if c["prec"] == "f32":
        o, E, Eh = P.case_run(c), None, None
    else:
        o, E, Eh = P.envelope_f64(c["gsz"], c["pc"], c["coef"], state, c["K"], b, p, eps=1e-30)
    TN._close(c, g, o, E, Eh)
    assert g["X"].tobytes() == PP.unpad(g["P"]).tobytes()
    L = g["launches"]
    assert L["bc_mirror"] > 0 and L["jacobi2"] == L["jacobi3"] == L["rbsor2"] == L["rbsor4"] == 0, L
    assert g["info"]["periodic"] == P.bits(state[1]) and g["info"]["neumann"] == N.bits(state[0]) and g["info"]["cg_fused"] == 0
    if c["pc"] in ("mg", "mgrb"):
        assert g["info"]["mg_cycles"] == c["K"]


COUNT_IDS = [f"{s}_{a}_{w}" for s in ("px", "pxz") for a, w in P.COUNT_RUNS]


@pytest.mark.parametrize("s,pc,coef", [(s, a, w) for s in ("px", "pxz") for a, w in P.COUNT_RUNS], ids=COUNT_IDS)
def test_iteration_counts_to_convergence(s, pc, coef):
    """33 x 47 x 61, FP64, eps 1e-5: the counts tests/test_periodic_oracle.py records"""
    c = dict(gsz=P.COUNT_BOX, prec="f64", pc=pc, coef=coef, id=f"count_{pc}")
    b, p = PP.problem(c["gsz"], "f64", 0)
    g = _pcg_gpu(c, b, p, P.COUNT_STATES[s], 1000, 1e-5)
    assert g["itr"] == P.COUNTS[s, pc, coef], (g["itr"], P.COUNTS[s, pc, coef])
    assert g["hist"][-1] < 1e-5


# ---- the singular problems: the channel and the triply periodic box, projected
@pytest.mark.parametrize("pc,coef", [("jacobi", 0.8), ("mg", 0.8), ("mgrb", 1.2)])
@pytest.mark.parametrize("s", ["channel", "triple"])
def test_singular_problems_converge_on_an_incompatible_rhs(s, pc, coef):
    """33 x 47 x 61 FP64 eps 1e-5 on the seeded (incompatible) b: the restatement's count, its mean of b, an answer whose mean lies inside
    closed_parity.mean_bound"""
    c = dict(gsz=P.COUNT_BOX, prec="f64", pc=pc, coef=coef, id=f"singular_{s}_{pc}")
    b, p = PP.problem(c["gsz"], "f64", 0)
    g = _pcg_gpu(c, b, p, P.STATES[s], 300, 1e-5)
    o = P.run(c["gsz"], pc, coef, "f64", P.STATES[s], 300, b, p, eps=1e-5)
    assert g["itr"] == o.itr == P.COUNTS[s, pc, coef] and g["hist"][-1] < 1e-5, (g["itr"], o.itr)
    assert abs(g["means"][0] - float(o.means[0])) <= o.mean_tol[0], (g["means"], o.means, o.mean_tol)
    x = g["X"][1:-1, 1:-1, 1:-1]
    mean = math.fsum(x.ravel()) / x.size
    bound = CB.mean_bound(g["means"][2], np.abs(x).max(), np.float64)
    print(f"{s} {pc}: mean of the answer {mean:.3e}, bound {bound:.3e}, means {g['means']}")
    assert abs(mean) <= bound, (mean, bound)
    assert g["info"]["closed"] == 1 and g["info"]["neumann"] == 63 and g["info"]["periodic"] == P.bits(P.STATES[s][1])


# ---- decomposed runs on the LOCAL transport
@pytest.mark.parametrize("c,div,state", P.DECOMP, ids=[d[0]["id"] for d in P.DECOMP])
def test_decomposed_solve(c, div, state):
    """a periodic direction that the decomposition does not cut: the gathered result under the existing decomposed bar (FP32 bit for bit, FP64
    within the exact-dot envelope); mg: the cycle alone byte-equal to the single domain, with the unperiodic count of exchanges"""
    gsz, prec = c["gsz"], c["prec"]
    b, p = PP.problem(gsz, prec, 0)
    X = np.full(gsz, np.nan, dtype=b.dtype)
    sz, idx, ins, r = TN._cycle_rhs(prec, gsz)
    Z = np.zeros_like(r)

    def work(q):
        cz = _handle(prec, list(gsz) + ["pcg", 100, c["coef"], c["pc"]] + list(div), state)
        try:
            info0 = None
            if c["pc"] == "mg":
                loc = cz.local()
                (hi, hj, hk), (ni, nj, nk) = loc["head"], loc["size"]
                z = cz.precondition(r[hj - 1:hj - 1 + nj + 2 * G, hi - 1:hi - 1 + ni + 2 * G, hk - 1:hk - 1 + nk + 2 * G])
                ist, ied, jst, jed, kst, ked = loc["inner"]
                Z[G + hj - 2 + jst:G + hj - 1 + jed, G + hi - 2 + ist:G + hi - 1 + ied, G + hk - 2 + kst:G + hk - 1 + ked] = \
                    z[G - 1 + jst:G + jed, G - 1 + ist:G + ied, G - 1 + kst:G + ked]
                info0 = cz.info()
            sl = cz.global_slice()
            cz.set_rhs(b[sl])
            cz.set_field(p[sl])
            itr = cz.solve()
            cz.get_field(X[sl])
            return itr, list(cz.history()), cz.info(), info0
        finally:
            cz.close()

    out = TN._ranks(prec, div, work)
    assert all(o[0] == out[0][0] and o[1] == out[0][1] for o in out)
    itr, hist = out[0][0], out[0][1]
    if c["pc"] == "mg":
        assert Z[ins].tobytes() == _cycle_gpu(prec, gsz, "mg", state).tobytes(), "the distributed cycle differs from the single-domain one"
        for o in out:
            assert o[3]["mg_exchanges"] == D.mg_exchanges(o[3]["mg_gather_level"]) and o[3]["periodic"] == P.bits(state[1]), o[3]
    if prec == "f32":
        o, E, Eh = P.run(gsz, c["pc"], c["coef"], prec, state, 100, b, p), None, None
    else:
        o, E, Eh = P.envelope_f64(gsz, c["pc"], c["coef"], state, 100, b, p)
    assert o.res < O.EPS and o.itr < 100
    TN._close(c, dict(itr=itr, hist=hist, P=PP.pad(X)), o, E, Eh)


# ---- a manufactured periodic solution, as a user would check the library
def test_manufactured_periodic_solution_pcg_mgrb_64_f64():
    """64^3 FP64, pcg 100 1.0 mgrb, eps 1e-10, periodic X and Z, Y+ zero-flux: a smooth u periodic in X and Z, b = A u by the oracle's
    blas_calc_ax on the filled field.  The bar of test_gpu_neumann.py::test_manufactured_solution_pcg_mgrb_64_f64: the GPU's max error against
    u is at most the restatement's plus 2 E + 8 ulp (E from the perturbed restated runs)"""
    gsz, state = (64, 64, 64), ((0, 0, 0, 1, 0, 0), P.PXZ, False)
    u, b, p = P.manufactured(gsz, state[0], state[1])
    c = dict(gsz=gsz, prec="f64", pc="mgrb", coef=1.0, id="manufactured")
    g = _pcg_gpu(c, b, p, state, 100, 1e-10)
    r = {q: P.run(gsz, "mgrb", 1.0, "f64", state, 100, b, p, eps=1e-10, perturb=q) for q in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr == g["itr"] < 100
    err = {q: float(np.abs(PP.unpad(r[q].P) - u).max()) for q in r}
    E = max(abs(err[1] - err[0]), abs(err[-1] - err[0]))
    gerr = float(np.abs(g["X"] - u).max())
    print("manufactured (periodic): restated error", err[0], "GPU error", gerr, "envelope", E, "iterations", g["itr"])
    assert gerr <= err[0] + 2.0 * E + 8.0 * np.spacing(np.abs(u).max())


# ---- mixed-precision refinement
REFINE_BOX, REFINE_STATE = (33, 47, 61), P.STATES["pxz_ym"]


def test_refined_periodic_reaches_1e10_in_the_restated_steps():
    from test_gpu_problem import _torch
    _torch()
    import refine_parity as RP
    from cubez_amd.refine import Refined
    b, p = PP.problem(REFINE_BOX, "f64", 0)
    want, hist, _, ratios = P.refine(b, p, REFINE_STATE, tol=1e-10)
    assert want > 0 and ratios[-1] <= 1e-10 and RP.premise(ratios, 1e-10, int(np.prod([n - 2 for n in REFINE_BOX])))
    R = Refined(REFINE_BOX, neumann=REFINE_STATE[0], periodic=REFINE_STATE[1])
    try:
        R.set_rhs(b)
        R.set_field(p)
        steps = R.solve(tol=1e-10)
        x = R.get_field()
        assert steps == want, (steps, R.history, hist)
        assert R.history[-1][1] <= 1e-10 and [h[2] for h in R.history] == [h[2] for h in hist]
        assert R.hi.info()["periodic"] == R.lo.info()["periodic"] == P.bits(REFINE_STATE[1])
        assert np.array_equal(x[0, 1:-1, 1:-1], x[-2, 1:-1, 1:-1]) and np.array_equal(x[-1, 1:-1, 1:-1], x[1, 1:-1, 1:-1])  # the X layers are the wrap
    finally:
        R.close()


def test_refinement_steps_through_host_arrays():
    """the loop of cubez_amd.refine.Refined written with host arrays (no torch): an FP64 handle that never solves, an FP32 pcg 1000 1.2 mgrb,
    the state on both; 1e-10 in the restated loop's outer steps, with its inner iteration counts"""
    import refine_parity as RP
    from cubez_amd.refine import INNER_EPS, scale_of
    gsz, state = REFINE_BOX, REFINE_STATE
    b, p = PP.problem(gsz, "f64", 0)
    want, hist, _, ratios = P.refine(b, p, state, tol=1e-10)
    assert want > 0 and ratios[-1] <= 1e-10 and RP.premise(ratios, 1e-10, int(np.prod([n - 2 for n in gsz])))
    hi = _handle("f64", list(gsz) + ["jacobi", 1, 0.8], state)
    lo = _handle("f32", list(gsz) + ["pcg", 1000, 1.2, "mgrb"], state)
    try:
        hi.set_rhs(b)
        hi.set_field(p)
        npts = int(np.prod([n - 2 for n in gsz]))
        _, ss0 = hi.get_residual()
        ss, steps, got = ss0, 0, []
        while True:
            scale = scale_of(ss, npts)
            r32, ss = hi.get_residual(dtype=np.float32, scale=scale)
            if math.sqrt(ss) <= 1e-10 * math.sqrt(ss0) or steps == 20:
                break
            lo.set_rhs(r32)
            lo.set_field(np.zeros(gsz, dtype=np.float32))
            lo.set_eps(INNER_EPS)
            inner = lo.solve()
            assert inner > 0
            hi.add_field(lo.get_field(), 1.0 / scale)
            steps += 1
            got.append(inner)
        assert steps == want and got == [h[2] for h in hist], (steps, got, hist)
        x = hi.get_field()
        assert np.array_equal(x[0, 1:-1, 1:-1], x[-2, 1:-1, 1:-1]) and np.array_equal(x[1:-1, 0, 1:-1], x[1:-1, 1, 1:-1])  # the wrap, the mirror
    finally:
        hi.close()
        lo.close()


# ---- refusals, state and the invariant of the face layers
def test_refusals_and_solvability(capfd):
    from cubez_amd import CZ
    three, six = (C.c_int * 3), (C.c_int * 6)
    cz = CZ("f32", quiet=True)
    try:
        assert cz.lib.cz_set_periodic(cz.h, three(1, 0, 0)) == 0  # before cz_setup
        assert cz.lib.cz_set_periodic(None, three(1, 0, 0)) == 0  # NULL handle
        assert cz.setup([9, 7, 12, "jacobi", 50, 0.8]) == 1
        assert cz.lib.cz_set_periodic(cz.h, None) == 0  # NULL flags
        assert cz.info()["periodic"] == 0
        # the rule on the combined state, through all three setters
        assert cz.lib.cz_set_periodic(cz.h, three(1, 1, 1)) == 0  # no Dirichlet face left, the closed mode off
        cz.set_neumann((0, 0, 1, 1, 1, 1))
        assert cz.lib.cz_set_periodic(cz.h, three(1, 0, 0)) == 0  # X periodic, Y and Z all Neumann
        cz.set_neumann((1, 1, 0, 1, 1, 1))
        cz.set_periodic((1, 0, 0))  # (the X flags are ignored, Y- is Dirichlet)
        assert cz.info()["periodic"] == 1 and cz.info()["neumann"] == N.bits((1, 1, 0, 1, 1, 1))
        assert cz.lib.cz_set_neumann(cz.h, six(0, 0, 1, 1, 1, 1)) == 0  # cz_set_neumann asks the same rule
        assert cz.info()["neumann"] == N.bits((1, 1, 0, 1, 1, 1))
        cz.set_closed_box(True)
        cz.set_periodic((1, 1, 1))  # the triply periodic box
        assert cz.info()["periodic"] == 7 and cz.info()["closed"] == 1 and cz.info()["neumann"] == 63
        assert cz.lib.cz_set_closed_box(cz.h, 0) == 0  # the closed mode off would leave no Dirichlet face
        assert cz.info()["closed"] == 1
        cz.set_periodic((1, 0, 1))  # the channel
        assert cz.lib.cz_set_closed_box(cz.h, 0) == 1  # Y's faces are Dirichlet faces again
        assert cz.info()["closed"] == 0 and cz.info()["neumann"] == 0 and cz.info()["periodic"] == 5
        # a solver other than pcg refuses to run and leaves P alone
        before = cz.field()
        assert cz.solve() == 0 and cz.sweeps(4) == 0
        assert cz.evaluate([9, 7, 12, "jacobi", 50, 0.8]) == 0
        assert cz.field().tobytes() == before.tobytes() and cz.info()["periodic"] == 5
        cz.set_periodic((0, 0, 0))
        assert cz.solve() > 0
    finally:
        cz.close()
    err = capfd.readouterr().err
    assert err.count("cz_set_periodic:") == 5 and err.count("cz_set_neumann:") == 1 and err.count("cz_set_closed_box:") == 1, err
    assert err.count("cz_set_closed_box") == 5, err  # each of the four refusals of the rule names the call that keeps the problem solvable
    assert err.count("cz_solve:") == 1 and err.count("cz_sweeps:") == 1 and err.count("cz_evaluate:") == 1, err
    # G_size < 4, a _maf handle
    thin, maf = CZ("f32", quiet=True), CZ("f32", quiet=True)
    try:
        assert thin.setup([3, 40, 40, "pcg", 10, 0.8, "mg"]) == 1
        assert thin.lib.cz_set_periodic(thin.h, three(1, 0, 0)) == 0 and thin.info()["periodic"] == 0
        thin.set_periodic((0, 1, 1))
        assert maf.setup([9, 7, 12, "jacobi_maf", 50, 0.8]) == 1
        assert maf.lib.cz_set_periodic(maf.h, three(1, 0, 0)) == 0
        with pytest.raises(ValueError):
            maf.set_periodic([1, 0])
        assert maf.solve() > 0
    finally:
        thin.close()
        maf.close()
    assert capfd.readouterr().err.count("cz_set_periodic:") == 2


def test_a_cut_direction_is_refused():
    """(2, 1, 1): X is cut, so periodic X is refused on every rank and periodic Y is taken"""
    def work(q):
        cz = _handle("f32", [32, 36, 40, "pcg", 10, 0.8, "jacobi", 2, 1, 1])
        try:
            refused = cz.lib.cz_set_periodic(cz.h, (C.c_int * 3)(1, 0, 0))
            kept = cz.info()["periodic"]
            cz.set_periodic((0, 1, 0))
            return refused, kept, cz.info()["periodic"]
        finally:
            cz.close()

    assert TN._ranks("f32", (2, 1, 1), work) == [(0, 0, 2), (0, 0, 2)]


def test_setup_clears_the_flags_and_off_gives_the_unflagged_bits():
    """cz_setup (through cz_evaluate) after the flags: the solve of a fresh handle; flags off again: the bytes of a handle that never saw
    them, the fused direction included"""
    from cubez_amd import CZ
    args = [33, 47, 61, "pcg", 100, 1.2, "mgrb"]
    ev, fresh = CZ("f64", quiet=True), CZ("f64", quiet=True)
    try:
        assert ev.setup(args) == 1
        ev.set_periodic((1, 0, 1))
        assert ev.evaluate(args) == 1 and ev.info()["periodic"] == 0
        assert fresh.evaluate(args) == 1
        assert ev.iter == fresh.iter and ev.field().tobytes() == fresh.field().tobytes() and ev.info()["cg_fused"] == ev.iter
    finally:
        ev.close()
        fresh.close()
    for pc, coef in (("mg", 0.8), ("mgrb", 1.2)):
        b, p = PP.problem((33, 47, 61), "f32", 0)
        a, plain = CZ("f32", quiet=True), CZ("f32", quiet=True)
        try:
            for cz in (a, plain):
                assert cz.setup([33, 47, 61, "pcg", 100, coef, pc]) == 1
                cz.set_rhs(b)
            a.set_periodic((1, 1, 0))
            a.set_field(p)
            assert a.solve() > 0
            a.set_periodic((0, 0, 0))
            for cz in (a, plain):
                cz.set_field(p)
            assert a.solve() == plain.solve() > 0
            assert a.field().tobytes() == plain.field().tobytes() and a.info()["cg_fused"] == a.iter
        finally:
            a.close()
            plain.close()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_face_layers_hold_the_wrap_after_every_call_that_writes_the_field(prec):
    """cz_set_periodic, cz_set_neumann, cz_set_field, cz_add_field and cz_solve: get_field returns the wrap in the periodic direction (whatever
    was passed there), the mirror on the Neumann face and the caller's values on the Dirichlet ones; the residual is 0 on every physical face"""
    gsz, faces, per = (9, 7, 12), (1, 0, 0, 0, 0, 1), P.PX  # X periodic (its Neumann flag ignored), Z+ zero-flux
    b, p = PP.problem(gsz, prec, 3)
    sz, idx = TN._box(gsz)

    def filled(a, f=faces):
        return PP.unpad(P.fill(PP.pad(a), sz, idx, f, per))

    cz = _handle(prec, list(gsz) + ["pcg", 5, 0.8, "mg"])
    try:
        cz.set_periodic(per)
        x = cz.get_field()  # cz_set_periodic wrapped the built-in field
        assert x.tobytes() == filled(x, N.NONE).tobytes() and np.array_equal(x[0, 1:-1, 1:-1], x[-2, 1:-1, 1:-1])
        cz.set_neumann(faces)
        x = cz.get_field()
        assert x.tobytes() == filled(x).tobytes() and np.array_equal(x[1:-1, 1:-1, -1], x[1:-1, 1:-1, -2])
        cz.set_rhs(b)
        cz.set_field(p)
        x = cz.get_field()
        assert x.tobytes() == filled(p).tobytes() and x.tobytes() != p.tobytes()
        assert np.array_equal(x[:, 0], p[:, 0]) and np.array_equal(x[:, -1], p[:, -1]) and np.array_equal(x[:, :, 0], p[:, :, 0])  # Dirichlet
        e = np.random.default_rng(4).random(gsz).astype(np.float32)
        cz.add_field(e, 0.5)
        want = p.copy()
        want[1:-1, 1:-1, 1:-1] = p[1:-1, 1:-1, 1:-1] + e.astype(p.dtype)[1:-1, 1:-1, 1:-1] * p.dtype.type(0.5)
        x = cz.get_field()
        assert x.tobytes() == filled(want).tobytes()
        r, ss = cz.get_residual(dtype=np.float64)
        k = P.kernels(prec, faces, per)
        rk = k.alloc(sz)
        k.blas_calc_rk(rk, PP.pad(x), PP.pad(b), sz, idx, np.array([1, 1, 1, 1, 1, 1, 6], dtype=k.real))
        assert r.tobytes() == PP.unpad(rk).astype(np.float64).tobytes() and ss > 0.0
        inner = np.zeros(gsz, dtype=bool)
        inner[1:-1, 1:-1, 1:-1] = True
        assert not r[~inner].any()
        assert cz.solve() > 0
        x = cz.get_field()
        assert x.tobytes() == filled(x).tobytes()
        assert np.array_equal(x[:, 0], p[:, 0]) and np.array_equal(x[:, -1], p[:, -1]) and np.array_equal(x[:, :, 0], p[:, :, 0])
    finally:
        cz.close()
