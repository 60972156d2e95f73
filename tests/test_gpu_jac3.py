"""GPU tests (-m gpu) of the three-sweep Jacobi pass (jac3_k, czhip_jacobi3_async): the kernel against three oracle sweeps, the driver's
triples against one and two sweeps per pass and against the oracle -- fields bit for bit, residuals to the double-summation tolerance."""
import numpy as np
import pytest

from oracle import cz_oracle as O

pytestmark = pytest.mark.gpu

BOXES = [((40, 36, 60), None), ((33, 70, 124), None), ((130, 20, 252), None), ((24, 20, 28), (1, 24, 1, 20, 1, 28)), ((96, 40, 508), None),
         # rows that are no multiple of the vector width (nk + 4 = 65, 127, 63)
         ((40, 36, 61), None), ((33, 50, 123), None), ((24, 20, 59), (1, 24, 1, 20, 1, 59)),
         # rows cut into k windows
         ((9, 7, 1100), None), ((7, 6, 2100), None)]
FORMS = [(0, 0), (5, 0), (9, 3), (32, 2), (0, 7)]  # (vectors per k window, planes per chunk); 0 = the launcher's rule


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("unit", [0, 1], ids=["coef", "unit"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("box", BOXES, ids=[f"{b[0][0]}x{b[0][1]}x{b[0][2]}{'' if b[1] is None else '_idx'}" for b in BOXES])
def test_three_sweeps_per_pass_equal_three_oracle_sweeps(prec, box, unit):
    """czhip_jacobi3_async == three jacobi sweeps of the oracle, bit for bit, with the residuals of all three sweeps; windows of 5 / 9 / 32
    vectors and the launcher's own, chunks of 2, 3, 7 planes; general and unit coefficients.  The input is never modified."""
    from cubez_amd import CzHip
    (ni, nj, nk), idx = box
    sz = [ni, nj, nk]
    idx = list(idx) if idx else [2, ni - 1, 2, nj - 1, 2, nk - 1]
    h, ko = CzHip(prec), O.Kernels("oracle", prec)
    R = ko.real
    rng = np.random.default_rng(5 * ni + 7 * nj + 3 * nk + unit)
    shape = (nj + 4, ni + 4, nk + 4)
    if unit:
        cf = np.array([1, 1, 1, 1, 1, 1, 6], dtype=R)
    else:
        cf = rng.uniform(0.5, 1.5, 7).astype(R)
        cf[6] = 6.2
    p, b = (rng.uniform(-1, 1, shape).astype(R) for _ in range(2))
    a, w, r = p.copy(), np.zeros_like(p), []
    for _ in range(3):
        wide = np.zeros(1)
        ko.jacobi(a, sz, idx, cf, 0.9, b, w, wide=wide)
        r.append(wide[0])
    du, db = h.alloc(sz, p), h.alloc(sz, b)
    launched = 0
    try:
        for kw, tj in FORMS:
            assert h.lib.czhip_set_jac3(2, kw, tj) == 0
            dw = h.alloc(sz, p)
            ok, r1, r2, r3 = h.jacobi3(du, dw, db, sz, idx, cf, 0.9)
            if ok:
                launched += 1
                assert dw.get().tobytes() == a.tobytes(), (kw, tj)
                assert du.get().tobytes() == p.tobytes()
                for got, want in zip((r1, r2, r3), r):
                    assert _rel(got, want) < 1e-11, (kw, tj, got, want)
            dw.free()
    finally:
        h.lib.czhip_set_jac3(1, 0, 0)
    assert launched > 0


def _solve(prec, gsz, itmax, coef, jac3, t2=1):
    from cubez_amd import CZ
    cz = CZ(prec, quiet=True)
    cz.lib.czhip_set_jac3(jac3, -1, -1)
    cz.lib.czhip_set_tuning2(0, 0, -1, t2)
    try:
        assert cz.setup(list(gsz) + ["jacobi", itmax, coef]) == 1
        itr = cz.solve()
        return dict(itr=itr, res=cz.res, hist=list(cz.history()), P=cz.field().tobytes(), info=cz.info())
    finally:
        cz.lib.czhip_set_jac3(1, -1, -1)
        cz.lib.czhip_set_tuning2(0, 0, -1, 1)
        cz.close()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz,coef,converged,reruns", [((16, 16, 16), 0.7, 361, 1), ((16, 16, 16), 0.8, 323, 1), ((18, 16, 20), 1.0, 312, 0)],
                         ids=["first", "second", "third"])
def test_jacobi_three_sweeps_per_pass_to_convergence_vs_oracle(prec, gsz, coef, converged, reruns):
    """Triples forced on (mode 2): passes start at iterations 1, 4, 7, ...  A solve converged at the first sweep of a triple (361) re-runs one
    sweep from the pass's input, at the second (323) one pair, at the third (312) nothing.  Iteration count, field bit for bit and history
    against the oracle and against the pair path (mode 0)."""
    g = _solve(prec, gsz, 100000, coef, 2)
    p = _solve(prec, gsz, 100000, coef, 0)
    o = O.run(gsz, "jacobi", 100000, coef, None, kind="oracle", prec=prec, wide=True)
    assert o.itr == converged and g["itr"] == converged and p["itr"] == converged
    assert g["info"]["pass_kind"] == 1 and g["info"]["jac3_passes"] > 0 and p["info"]["jac3_passes"] == 0, (g["info"], p["info"])
    assert g["info"]["exact_reruns"] == reruns, g["info"]
    assert g["P"] == o.P.tobytes() and g["P"] == p["P"]
    assert np.allclose(g["hist"], [r for _, r in o.history], rtol=1e-11, atol=0)
    assert np.allclose(g["hist"], p["hist"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("itmax", [1, 2, 4, 5, 7])
def test_jacobi_fixed_iteration_counts_under_triples(prec, itmax):
    """Fixed ItrMax: triples while three sweeps remain, then a pair or a single sweep -- the same field as single sweeps and the oracle."""
    gsz = (40, 36, 44)
    g = _solve(prec, gsz, itmax, 0.8, 2)
    s = _solve(prec, gsz, itmax, 0.8, 0, t2=0)
    o = O.run(gsz, "jacobi", itmax, 0.8, None, kind="oracle", prec=prec, wide=True)
    assert g["itr"] == s["itr"] == o.itr == itmax + 1
    assert g["info"]["jac3_passes"] == itmax // 3, g["info"]
    assert g["P"] == s["P"] == o.P.tobytes()
    assert np.allclose(g["hist"], s["hist"], rtol=1e-12, atol=0)
    assert np.allclose(g["hist"], [r for _, r in o.history], rtol=1e-11, atol=0)


def test_jacobi_triples_stay_off_on_small_grids_by_default():
    g = _solve("f32", (40, 36, 44), 7, 0.8, 1)
    assert g["info"]["jac3_passes"] == 0


def test_bench_leg_sweeps_equal_solver_sweeps_under_triples():
    """cz_sweeps (bench.py's timed region) under triples: 7 + 6 bench sweeps == 13 solver iterations."""
    from cubez_amd import CZ
    runs = []
    for bench in (False, True):
        cz = CZ("f32", quiet=True)
        cz.lib.czhip_set_jac3(2, -1, -1)
        try:
            assert cz.setup([40, 36, 44, "jacobi", 13, 0.8]) == 1
            if bench:
                cz.sweeps(7), cz.sweeps(6)
            else:
                assert cz.solve() == 14
            assert cz.info()["jac3_passes"] > 0
            runs.append((cz.field().tobytes(), cz.res))
        finally:
            cz.lib.czhip_set_jac3(1, -1, -1)
            cz.close()
    assert runs[0][0] == runs[1][0]
    assert abs(runs[0][1] - runs[1][1]) <= 1e-12 * runs[0][1]


@pytest.mark.parametrize("nit", [4, 7])
def test_jacobi_512_triples_against_oracle(nit):
    """`cz 512 512 512 jacobi` (the headline workload) takes the triple by default: == the oracle, bit for bit, history to 1e-11."""
    N = 512
    g = _solve("f32", (N, N, N), nit, 0.8, 1)
    assert g["info"]["jac3_passes"] == nit // 3 and g["info"]["pass_kind"] == 1, g["info"]
    o = O.run((N, N, N), "jacobi", nit, 0.8, kind="oracle", prec="f32", wide=True)
    assert g["itr"] == o.itr == nit + 1
    assert g["P"] == o.P.tobytes()
    assert np.allclose(g["hist"], [r for _, r in o.history], rtol=1e-11, atol=0)
