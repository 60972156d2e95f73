"""Zero-flux (Neumann) faces for pcg on the GPU (-m gpu), every result against the restatement of tests/neumann_parity.py:
the mirror kernel alone; the V-cycles with the masked coarse diagonal (cz_precondition, byte for byte, CZ_MG_TAIL 0 and 1); PCG iteration by
iteration on a caller's problem against the exact-dot oracle; decomposed runs on the LOCAL transport; a manufactured solution; mixed-precision
refinement; the refusals and the invariant of the face layers."""
import ctypes as C
import os
import subprocess
import sys
import textwrap
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_parity as M  # noqa: E402
import neumann_parity as N  # noqa: E402
import problem_parity as PP  # noqa: E402
from cubez_amd import decomp as D  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = O.GUIDE
OMG = {"mg": 0.8, "mgrb": 1.2}


def _real(prec):
    return np.float32 if prec == "f32" else np.float64


def _box(gsz):
    idx, _ = O.range_inner_index(list(gsz), [-1] * 6)
    return list(gsz), idx


def _handle(prec, args, faces=None):
    from cubez_amd import CZ
    cz = CZ(prec, quiet=True)
    assert cz.setup(list(args)) == 1
    if faces is not None:
        cz.set_neumann(faces)
    return cz


# ---- the mirror kernel alone
MIRROR_MASKS = {"xm": N.X_MINUS, "xp_ym_zp": N.MIXED, "five": N.FIVE}


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("mask", list(MIRROR_MASKS))
@pytest.mark.parametrize("gsz", [(9, 7, 12), (33, 47, 61), (40, 40, 1100)], ids=["9x7x12", "33x47x61", "40x40x1100"])
def test_mirror_kernel_writes_the_named_face_cells_only(gsz, mask, prec):
    """czhip_mirror_faces_async on an array full of random numbers: the named face cells take the first inner layer, every other byte
    (edges, corners, guide cells, the other faces) stays; a face that is rank-internal by the brick's index range is not touched"""
    from cubez_amd.lib import CzHip
    hip = CzHip(prec)
    faces = MIRROR_MASKS[mask]
    sz, idx = _box(gsz)
    host = np.random.default_rng(21).random((gsz[1] + 2 * G, gsz[0] + 2 * G, gsz[2] + 2 * G)).astype(hip.real)
    d = hip.alloc(sz, host)
    try:
        hip.timing(True)
        assert hip.mirror_faces(d, sz, idx, faces)
        want = N.mirror(host.copy(), sz, idx, faces)
        assert not np.array_equal(want, host)
        assert d.get().tobytes() == want.tobytes()
        # the index range of a brick whose - sides are rank-internal: those faces are left alone whatever the mask says
        d.put(host)
        idx_b = [1, idx[1], 1, idx[3], 1, idx[5]]
        assert hip.mirror_faces(d, sz, idx_b, faces)
        assert d.get().tobytes() == N.mirror(host.copy(), sz, idx_b, faces).tobytes()
        # one launch per call whatever the number of faces, none where no flagged face is physical (the second call of the X- mask)
        assert hip.timing_read("bc_mirror")[0] == 1 + int(any(faces[f] for f in (1, 3, 5)))
    finally:
        hip.timing(False)
        hip.sync()
        d.free()


# ---- the V-cycles with a mask: cz_precondition against the restatement
CYCLE_BOXES = [(9, 7, 12), (33, 47, 61), (3, 40, 40), (64, 64, 64)]
CYCLE_MASKS = ("z", "five")


def _cycle_rhs(prec, gsz):
    sz, idx = _box(gsz)
    r = np.zeros((gsz[1] + 2 * G, gsz[0] + 2 * G, gsz[2] + 2 * G), dtype=_real(prec))
    ins = M.inner(sz, idx)
    r[ins] = np.random.default_rng(23).standard_normal(r[ins].shape).astype(r.dtype)
    return sz, idx, ins, r


def _cycle_gpu(prec, gsz, kind, faces):
    sz, idx, ins, r = _cycle_rhs(prec, gsz)
    cz = _handle(prec, list(gsz) + ["pcg", 1, OMG[kind], kind], faces)
    try:
        z = cz.precondition(r)
        assert cz.precondition(r).tobytes() == z.tobytes(), "the second cycle differs"
        assert cz.info()["neumann"] == N.bits(faces)
        return z[ins]
    finally:
        cz.close()


_TAIL0_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
    import numpy as np
    import test_gpu_neumann as T
    out = {{}}
    for gsz in T.CYCLE_BOXES:
        for prec in ("f32", "f64"):
            for kind in ("mg", "mgrb"):
                for mask in T.CYCLE_MASKS:
                    out["_".join(map(str, gsz)) + prec + kind + mask] = T._cycle_gpu(prec, gsz, kind, T.N.MASKS[mask])
    np.savez({path!r}, **out)
    """)


@pytest.fixture(scope="module")
def tail0(tmp_path_factory):
    """every cycle case with CZ_MG_TAIL=0, computed once in a child process (the variable is read when the hierarchy is created)"""
    path = str(tmp_path_factory.mktemp("neumann") / "tail0.npz")
    env = dict(os.environ, CZ_MG_TAIL="0")
    p = subprocess.run([sys.executable, "-c", _TAIL0_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return np.load(path)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", CYCLE_BOXES, ids=["x".join(map(str, g)) for g in CYCLE_BOXES])
def test_precondition_with_a_mask_equals_the_restatement(gsz, prec, tail0):
    """mg and mgrb, the masks Z+- and five faces: byte for byte, the tail kernel and the level kernels giving equal bits ((3, 40, 40): a level of
    one point in x; with the five-face mask it lies between two Neumann faces)"""
    sz, idx, ins, r = _cycle_rhs(prec, gsz)
    for kind in ("mg", "mgrb"):
        for mask in CYCLE_MASKS:
            faces = N.MASKS[mask]
            k = N.Kernels("oracle", prec)
            k.faces = faces
            ref = N.apply(kind, k, r, sz, idx, OMG[kind], faces)[ins]
            z = _cycle_gpu(prec, gsz, kind, faces)
            assert z.tobytes() == ref.tobytes(), (kind, mask)
            assert tail0["_".join(map(str, gsz)) + prec + kind + mask].tobytes() == z.tobytes(), f"{kind} {mask}: CZ_MG_TAIL=0 changed the bits"


# ---- PCG on a caller's problem, K iterations against the exact-dot restatement
def _pcg_gpu(c, b, p, faces, itr_max, eps, division=None):
    cz = _handle(c["prec"], list(c["gsz"]) + ["pcg", itr_max, c["coef"], c["pc"]] + (list(division) if division else []))
    try:
        cz.timing(True)
        if faces is not None:
            cz.set_neumann(faces)
        cz.set_rhs(b)
        cz.set_field(p)
        cz.set_eps(eps)
        itr = cz.solve()
        return dict(itr=itr, hist=list(cz.history()), P=cz.field(), X=cz.get_field(), info=cz.info(), launches=cz.launches())
    finally:
        cz.timing(False)
        cz.close()


def _close(c, g, o, E, Eh):
    assert g["itr"] == o.itr, (c["id"], g["itr"], o.itr)
    h0 = [r for _, r in o.history]
    if c["prec"] == "f32":
        assert g["hist"] == h0, c["id"]
        assert g["P"].tobytes() == o.P.tobytes(), f"{c['id']}: field differs from the restatement"
    else:
        ok, worst = PP.f64_close(g["P"], o.P, E)
        assert ok, f"{c['id']}: field beyond 2 E + 8 ulp (worst |d| / bound = {worst:.3g})"
        assert len(g["hist"]) == len(h0)
        ok, worst = PP.f64_close(g["hist"], h0, Eh)
        assert ok, f"{c['id']}: history beyond 2 E + 8 ulp (worst |d| / bound = {worst:.3g})"


@pytest.mark.parametrize("c", N.PCG_CASES, ids=[c["id"] for c in N.PCG_CASES])
def test_pcg_iterations_vs_exact_dot_restatement(c):
    """FP32: count, history and the whole padded field bit for bit; FP64: within 2 E + 8 ulp (problem_parity.f64_close); the masked handle runs
    mirrors and none of the fused pairs"""
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    g = _pcg_gpu(c, b, p, c["faces"], c["K"], 1e-30)
    if c["prec"] == "f32":
        o, E, Eh = N.case_run(c), None, None
    else:
        o, E, Eh = N.envelope_f64(c["gsz"], c["pc"], c["coef"], c["faces"], c["K"], b, p, eps=1e-30)
    _close(c, g, o, E, Eh)
    assert g["X"].tobytes() == PP.unpad(g["P"]).tobytes()
    L = g["launches"]
    assert L["bc_mirror"] > 0 and L["jacobi2"] == L["jacobi3"] == L["rbsor2"] == L["rbsor4"] == 0, L
    assert g["info"]["neumann"] == N.bits(c["faces"]) and g["info"]["cg_fused"] == 0
    if c["pc"] in ("mg", "mgrb"):
        assert g["info"]["mg_cycles"] == c["K"]


@pytest.mark.parametrize("pc,coef", [("mg", 0.8), ("mgrb", 1.2)])
def test_a_handle_without_a_mask_runs_no_mirror(pc, coef):
    c = dict(gsz=(33, 47, 61), prec="f32", pc=pc, coef=coef, id="nomask")
    b, p = PP.problem(c["gsz"], "f32", 0)
    g = _pcg_gpu(c, b, p, None, 3, 1e-30)
    assert g["launches"]["bc_mirror"] == 0 and g["info"]["neumann"] == 0 and g["info"]["cg_fused"] == 3, (g["launches"], g["info"])


@pytest.mark.parametrize("pc,coef", N.COUNT_RUNS, ids=[f"{a}_{w}" for a, w in N.COUNT_RUNS])
def test_iteration_counts_to_convergence(pc, coef):
    """33 x 47 x 61, FP64, five Neumann faces, eps 1e-5: the counts tests/test_neumann_oracle.py records"""
    c = dict(gsz=(33, 47, 61), prec="f64", pc=pc, coef=coef, id=f"count_{pc}")
    b, p = PP.problem(c["gsz"], "f64", 0)
    g = _pcg_gpu(c, b, p, N.FIVE, 1000, 1e-5)
    assert g["itr"] == N.COUNTS["five", pc, coef], (g["itr"], N.COUNTS["five", pc, coef])
    assert g["hist"][-1] < 1e-5


# ---- decomposed runs on the LOCAL transport
def _ranks(prec, div, work):
    """work(cz-less rank index) on every rank as a thread; returns the list of results"""
    from cubez_amd import load
    lib = load(prec)
    lib.cz_comm_local_world.restype = C.c_void_p
    lib.cz_comm_bootstrap_local.argtypes = [C.c_void_p, C.c_int]
    lib.cz_comm_local_world_free.argtypes = [C.c_void_p]
    n = div[0] * div[1] * div[2]
    world = lib.cz_comm_local_world(n)
    out, errors = [None] * n, []

    def run(q):
        try:
            lib.cz_comm_bootstrap_local(world, q)
            out[q] = work(q)
        except BaseException as e:  # noqa: BLE001
            errors.append((q, repr(e)))

    th = [threading.Thread(target=run, args=(q,)) for q in range(n)]
    [t.start() for t in th]
    [t.join(timeout=90) for t in th]
    if any(t.is_alive() for t in th):  # a rank stuck in a collective cannot be unblocked (as tests/test_gpu_decomp.py)
        sys.stderr.write(f"DEADLOCK: decomposed Neumann run {div} did not finish in 90 s\n")
        sys.stderr.flush()
        os._exit(3)
    assert not errors, errors
    lib.cz_comm_local_world_free(world)
    return out


DECOMP = N.DECOMP


@pytest.mark.parametrize("c,div,faces", DECOMP, ids=[d[0]["id"] for d in DECOMP])
def test_decomposed_solve(c, div, faces):
    """the gathered result of a decomposed solve under the existing decomposed bar (FP32 bit for bit, FP64 within the exact-dot envelope: the
    all-reduce is one more summation order); mg: the cycle alone byte-equal to the single domain and with the unmasked count of exchanges"""
    gsz, prec = c["gsz"], c["prec"]
    b, p = PP.problem(gsz, prec, 0)
    X = np.full(gsz, np.nan, dtype=b.dtype)
    sz, idx, ins, r = _cycle_rhs(prec, gsz)
    Z = np.zeros_like(r)

    def work(q):
        cz = _handle(prec, list(gsz) + ["pcg", 100, c["coef"], c["pc"]] + list(div), faces)
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

    out = _ranks(prec, div, work)
    assert all(o[0] == out[0][0] and o[1] == out[0][1] for o in out)
    itr, hist = out[0][0], out[0][1]
    if c["pc"] == "mg":
        assert Z[ins].tobytes() == _cycle_gpu(prec, gsz, "mg", faces).tobytes(), "the distributed cycle differs from the single-domain one"
        for o in out:
            assert o[3]["mg_exchanges"] == D.mg_exchanges(o[3]["mg_gather_level"]) and o[3]["neumann"] == N.bits(faces), o[3]
    if prec == "f32":
        o, E, Eh = N.run(gsz, c["pc"], c["coef"], prec, faces, 100, b, p), None, None
    else:
        o, E, Eh = N.envelope_f64(gsz, c["pc"], c["coef"], faces, 100, b, p)
    assert o.res < O.EPS and o.itr < 100
    _close(c, dict(itr=itr, hist=hist, P=PP.pad(X)), o, E, Eh)


# ---- a manufactured solution, as a user would check the library
def test_manufactured_solution_pcg_mgrb_64_f64():
    """64^3 FP64, pcg 100 1.0 mgrb, eps 1e-10, Z+- and X+ zero-flux: a smooth u mirrored onto those faces, b = A u by the oracle's blas_calc_ax.
    The bar of test_gpu_problem.py::test_manufactured_solution_pcg_mgrb_64_f64: the GPU's max error against u is at most the restatement's plus
    2 E + 8 ulp (E from the perturbed restated runs)"""
    gsz, faces = (64, 64, 64), (0, 1, 0, 0, 1, 1)
    u, b, p = N.manufactured(gsz, faces)
    c = dict(gsz=gsz, prec="f64", pc="mgrb", coef=1.0, id="manufactured")
    g = _pcg_gpu(c, b, p, faces, 100, 1e-10)
    r = {q: N.run(gsz, "mgrb", 1.0, "f64", faces, 100, b, p, eps=1e-10, perturb=q) for q in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr == g["itr"] < 100
    err = {q: float(np.abs(PP.unpad(r[q].P) - u).max()) for q in r}
    E = max(abs(err[1] - err[0]), abs(err[-1] - err[0]))
    gerr = float(np.abs(g["X"] - u).max())
    print("manufactured (Neumann): restated error", err[0], "GPU error", gerr, "envelope", E, "iterations", g["itr"])
    assert gerr <= err[0] + 2.0 * E + 8.0 * np.spacing(np.abs(u).max())


# ---- mixed-precision refinement
REFINE_BOX, REFINE_MASK = (33, 47, 61), N.FIVE


@pytest.fixture(scope="module")
def refined_oracle():
    b, p = PP.problem(REFINE_BOX, "f64", 0)
    want, hist, _, ratios = N.refine(b, p, REFINE_MASK, tol=1e-10)
    import refine_parity as RP
    assert want > 0 and ratios[-1] <= 1e-10 and RP.premise(ratios, 1e-10, int(np.prod([n - 2 for n in REFINE_BOX])))
    return b, p, want, hist


def test_refinement_steps_through_host_arrays(refined_oracle):
    """the loop of cubez_amd.refine.Refined written with host arrays (no torch): an FP64 handle that never solves, an FP32 pcg 1000 1.2 mgrb,
    the mask on both; 1e-10 in the restated loop's outer steps, with its inner iteration counts"""
    import math
    from cubez_amd.refine import INNER_EPS, scale_of
    b, p, want, hist = refined_oracle
    gsz, faces = REFINE_BOX, REFINE_MASK
    hi = _handle("f64", list(gsz) + ["jacobi", 1, 0.8], faces)
    lo = _handle("f32", list(gsz) + ["pcg", 1000, 1.2, "mgrb"], faces)
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
        assert np.array_equal(x[0, 1:-1, 1:-1], x[1, 1:-1, 1:-1])  # the X- layer is the mirror
    finally:
        hi.close()
        lo.close()


def test_refined_with_a_mask_reaches_1e10_in_the_restated_steps(refined_oracle):
    from test_gpu_problem import _torch
    _torch()
    from cubez_amd.refine import Refined
    b, p, want, hist = refined_oracle
    R = Refined(REFINE_BOX, neumann=REFINE_MASK)
    try:
        R.set_rhs(b)
        R.set_field(p)
        steps = R.solve(tol=1e-10)
        x = R.get_field()
        assert steps == want, (steps, R.history, hist)
        assert R.history[-1][1] <= 1e-10 and [h[2] for h in R.history] == [h[2] for h in hist]
        assert R.hi.info()["neumann"] == R.lo.info()["neumann"] == N.bits(REFINE_MASK)
        assert np.array_equal(x[0, 1:-1, 1:-1], x[1, 1:-1, 1:-1])  # the X- layer is the mirror
    finally:
        R.close()


# ---- refusals and the invariant of the face layers
def test_refusals_leave_the_handle_usable(capfd):
    from cubez_amd import CZ
    six = (C.c_int * 6)
    cz = CZ("f32", quiet=True)
    try:
        assert cz.lib.cz_set_neumann(cz.h, six(0, 0, 0, 0, 1, 1)) == 0  # before cz_setup
        assert cz.setup([9, 7, 12, "jacobi", 50, 0.8]) == 1
        assert cz.lib.cz_set_neumann(cz.h, six(1, 1, 1, 1, 1, 1)) == 0  # all six
        assert cz.info()["neumann"] == 0
        o = O.run((9, 7, 12), "jacobi", 50, 0.8, kind="oracle", prec="f32", wide=True)
        assert cz.solve() == o.itr and cz.field().tobytes() == o.P.tobytes()  # the built-in problem, untouched by the refusals
        # accepted on a handle of another solver, which then refuses to solve and leaves P alone
        cz.set_neumann(N.Z_BOTH)
        before = cz.field()
        assert cz.info()["neumann"] == N.bits(N.Z_BOTH)
        assert cz.solve() == 0 and cz.sweeps(4) == 0
        assert cz.evaluate([9, 7, 12, "jacobi", 50, 0.8]) == 0 and cz.evaluate([9, 7, 12, "sor2sma", 50, 1.5]) == 0
        assert cz.field().tobytes() == before.tobytes() and cz.info()["neumann"] == N.bits(N.Z_BOTH)
        cz.set_neumann(N.NONE)
        assert cz.solve() > 0
    finally:
        cz.close()
    # cz_evaluate of pcg on a masked handle is accepted; its set-up starts with Dirichlet faces again (mask cleared, the unmasked solve)
    ev, fresh = CZ("f64", quiet=True), CZ("f64", quiet=True)
    try:
        args = [9, 7, 12, "pcg", 100, 0.8, "mg"]
        assert ev.setup(args) == 1
        ev.set_neumann(N.FIVE)
        assert ev.evaluate(args) == 1 and ev.info()["neumann"] == 0
        assert fresh.evaluate(args) == 1
        assert ev.iter == fresh.iter and ev.field().tobytes() == fresh.field().tobytes()
        assert ev.info()["cg_fused"] == ev.iter  # (the fused direction pass: no mask anywhere)
    finally:
        ev.close()
        fresh.close()
    maf = CZ("f32", quiet=True)
    try:
        assert maf.setup([9, 7, 12, "jacobi_maf", 50, 0.8]) == 1
        assert maf.lib.cz_set_neumann(maf.h, six(0, 0, 0, 0, 1, 1)) == 0
        with pytest.raises(ValueError):
            maf.set_neumann([0, 0, 0, 0, 1])
        assert maf.solve() > 0
    finally:
        maf.close()
    err = capfd.readouterr().err
    assert err.count("cz_set_neumann:") == 3 and err.count("cz_solve:") == 1 and err.count("cz_sweeps:") == 1, err
    assert err.count("cz_evaluate:") == 2, err


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_face_layers_hold_the_mirror_after_every_call_that_writes_the_field(prec):
    """set_field, add_field and solve: get_field returns mirrors on Neumann faces (whatever was passed there) and the caller's values on the
    Dirichlet ones; the residual is 0 on every physical face"""
    gsz, faces = (9, 7, 12), N.MIXED  # X+ Y- Z+
    b, p = PP.problem(gsz, prec, 3)
    sz, idx = _box(gsz)

    def mirrored(a):
        return PP.unpad(N.mirror(PP.pad(a), sz, idx, faces))

    cz = _handle(prec, list(gsz) + ["pcg", 5, 0.8, "mg"], faces)
    try:
        x = cz.get_field()  # cz_set_neumann mirrored the built-in field
        assert x.tobytes() == mirrored(x).tobytes()
        cz.set_rhs(b)
        cz.set_field(p)
        x = cz.get_field()
        assert x.tobytes() == mirrored(p).tobytes() and x.tobytes() != p.tobytes()
        assert np.array_equal(x[0], p[0]) and np.array_equal(x[:, -1], p[:, -1]) and np.array_equal(x[:, :, 0], p[:, :, 0])  # the Dirichlet faces
        e = np.random.default_rng(4).random(gsz).astype(np.float32)
        cz.add_field(e, 0.5)
        want = p.copy()
        want[1:-1, 1:-1, 1:-1] = p[1:-1, 1:-1, 1:-1] + e.astype(p.dtype)[1:-1, 1:-1, 1:-1] * p.dtype.type(0.5)
        x = cz.get_field()
        assert x.tobytes() == mirrored(want).tobytes()
        r, ss = cz.get_residual(dtype=np.float64)
        k = N.Kernels("oracle", prec)
        k.faces = faces
        rk = k.alloc(sz)
        k.blas_calc_rk(rk, PP.pad(x), PP.pad(b), sz, idx, np.array([1, 1, 1, 1, 1, 1, 6], dtype=k.real))
        assert r.tobytes() == PP.unpad(rk).astype(np.float64).tobytes() and ss > 0.0
        inner = np.zeros(gsz, dtype=bool)
        inner[1:-1, 1:-1, 1:-1] = True
        assert not r[~inner].any()
        assert cz.solve() > 0
        x = cz.get_field()
        assert x.tobytes() == mirrored(x).tobytes()
        assert np.array_equal(x[0], p[0]) and np.array_equal(x[:, -1], p[:, -1]) and np.array_equal(x[:, :, 0], p[:, :, 0])
    finally:
        cz.close()
