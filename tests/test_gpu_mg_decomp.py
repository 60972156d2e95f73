"""The distributed V-cycle of `pcg ... mg` on the GPU (-m gpu; DESIGN.md §5.10 "Decomposed runs"): ranks as threads on the LOCAL transport
(and two RCCL processes), every result against the single-domain run or the exact-dot oracle.

1. the cycle alone: cz_precondition on every brick = the single-domain cycle of the whole field, byte for byte, for every gather level and
   CZ_MG_TAIL 0 / 1;
2. PCG iteration by iteration against tests/mg_parity.run (FP32 bit for bit, FP64 within tests/test_gpu_pcg.py's bounds);
3. two RCCL processes: field and history byte-equal to the single-domain run;
4. whole solves take the oracle's iteration counts."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_parity as M  # noqa: E402
from cubez_amd import decomp as D  # noqa: E402
from test_gpu_pcg import _check, _f64_close  # noqa: E402

pytestmark = pytest.mark.gpu
OMG = 0.8
G = 2  # guide cells


class _env:
    """set environment variables for the CZ objects created inside (their configuration is read at creation), restore afterwards"""

    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _args(gsz, div=None, itmax=1):
    return list(gsz) + ["pcg", itmax, OMG, "mg"] + (list(div) if div else [])


def _single_z(prec, gsz, r):
    from cubez_amd import CZ
    cz = CZ(prec, quiet=True)
    try:
        assert cz.setup(_args(gsz)) == 1
        return cz.precondition(r), cz.info()
    finally:
        cz.close()


def _decomposed_z(prec, gsz, div, r):
    """cz_precondition on every brick (LOCAL transport); the bricks' owned inner points assembled into a global array"""
    from cubez_amd import CZ, load
    import ctypes as C
    lib = load(prec)
    lib.cz_comm_local_world.restype = C.c_void_p
    lib.cz_comm_bootstrap_local.argtypes = [C.c_void_p, C.c_int]
    lib.cz_comm_local_world_free.argtypes = [C.c_void_p]
    n = div[0] * div[1] * div[2]
    world = lib.cz_comm_local_world(n)
    out, errors = [None] * n, []

    def work(q):
        try:
            lib.cz_comm_bootstrap_local(world, q)
            cz = CZ(prec, quiet=True)
            try:
                assert cz.setup(_args(gsz, div)) == 1
                loc = cz.local()
                (hi, hj, hk), (ni, nj, nk) = loc["head"], loc["size"]
                rl = r[hj - 1:hj - 1 + nj + 2 * G, hi - 1:hi - 1 + ni + 2 * G, hk - 1:hk - 1 + nk + 2 * G]
                z1 = cz.precondition(rl)
                z2 = cz.precondition(rl)  # a second cycle: the same bits (nothing of the first one is read)
                assert z1.tobytes() == z2.tobytes(), "the second cycle differs"
                out[q] = (z1, loc, cz.info())
            finally:
                cz.close()
        except BaseException as e:  # noqa: BLE001
            errors.append((q, repr(e)))

    th = [threading.Thread(target=work, args=(q,)) for q in range(n)]
    [t.start() for t in th]
    [t.join(timeout=90) for t in th]
    if any(t.is_alive() for t in th):
        sys.stderr.write(f"DEADLOCK: distributed V-cycle {gsz} {div} did not finish in 90 s\n")
        sys.stderr.flush()
        os._exit(3)
    assert not errors, errors
    lib.cz_comm_local_world_free(world)
    Z = np.zeros_like(r)
    for z, loc, _ in out:
        ist, ied, jst, jed, kst, ked = loc["inner"]
        hi, hj, hk = loc["head"]
        Z[G + hj - 2 + jst:G + hj - 1 + jed, G + hi - 2 + ist:G + hi - 1 + ied, G + hk - 2 + kst:G + hk - 1 + ked] = \
            z[G - 1 + jst:G + jed, G - 1 + ist:G + ied, G - 1 + kst:G + ked]
    return Z, [o[2] for o in out]


CYCLE_CASES = [((33, 47, 61), (2, 1, 1)), ((33, 47, 61), (1, 2, 1)), ((33, 47, 61), (1, 1, 2)), ((33, 47, 61), (2, 2, 2)),
               ((33, 47, 61), (3, 1, 2)), ((64, 64, 64), (2, 2, 2)), ((6, 6, 6), (2, 1, 1)), ((40, 40, 9), (1, 1, 3))]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz,div", CYCLE_CASES, ids=[f"{'x'.join(map(str, g))}_{'x'.join(map(str, d))}" for g, d in CYCLE_CASES])
def test_distributed_cycle_equals_single_domain(gsz, div, prec):
    """byte for byte, with the default gather level, G forced to 1 and to its deepest value, and CZ_MG_TAIL=0; every variant with exactly
    the exchanges per cycle that the order of the cycle implies (the one observable of where the exchanges stand)"""
    R = np.float32 if prec == "f32" else np.float64
    rng = np.random.default_rng(3)
    r = np.zeros((gsz[1] + 4, gsz[0] + 4, gsz[2] + 4), dtype=R)
    r[G + 1:G + gsz[1] - 1, G + 1:G + gsz[0] - 1, G + 1:G + gsz[2] - 1] = rng.standard_normal((gsz[1] - 2, gsz[0] - 2, gsz[2] - 2)).astype(R)
    ref, info1 = _single_z(prec, gsz, r)
    ins = (slice(G + 1, G + gsz[1] - 1), slice(G + 1, G + gsz[0] - 1), slice(G + 1, G + gsz[2] - 1))
    levels = len(D.mg_level_dims(gsz))
    deepest = D.mg_gather_level(gsz, div, gather_points=0)
    variants = [dict(), dict(CZ_MG_GATHER=1 << 30), dict(CZ_MG_GATHER=0), dict(CZ_MG_TAIL=0, CZ_MG_GATHER=0)]
    seen = set()
    for env in variants:
        with _env(**env):
            Z, infos = _decomposed_z(prec, gsz, div, r)
        want_G = D.mg_gather_level(gsz, div, gather_points=int(env.get("CZ_MG_GATHER", D.MG_GATHER_DEFAULT)))
        for info in infos:
            assert info["mg_levels"] == info1["mg_levels"] == levels, info
            assert info["mg_gather_level"] == want_G, (env, info)
            assert info["mg_exchanges"] == D.mg_exchanges(want_G), (env, info)
        seen.add(want_G)
        assert Z[ins].tobytes() == ref[ins].tobytes(), f"{env}: the distributed cycle differs from the single-domain one (G = {want_G})"
    assert seen == ({1, deepest} if levels > 1 else {0})


# ---- PCG with the distributed cycle, iteration by iteration, against the exact-dot oracle
PCG_CASES = [c for c in M.CASES if c["gsz"] == (33, 47, 61)]


@pytest.mark.parametrize("div", [(2, 1, 2), (2, 2, 2)], ids=["2x1x2", "2x2x2"])
@pytest.mark.parametrize("c", PCG_CASES, ids=[c["id"] for c in PCG_CASES])
def test_decomposed_pcg_mg_vs_exact_dot_oracle(c, div, monkeypatch):
    """FP32: field, history and count bit for bit; FP64: within 2 E + 8 ulp (tests/test_gpu_pcg.py's bars)"""
    import test_gpu_pcg as TP
    from test_gpu_decomp import _decomposed
    monkeypatch.setattr(TP.CP, "oracle", M.oracle)
    monkeypatch.setattr(TP.CP, "envelope_f64", M.envelope_f64)
    monkeypatch.setattr(TP.CP, "premise_f32", lambda c, o, perturbed=False: M.premise_f32(c, o))

    def run(c, itr_max):
        results, Gf = _decomposed(c["prec"], c["gsz"], "pcg", itr_max, c["coef"], div, "mg")
        assert all(r[0] == results[0][0] and r[2] == results[0][2] for r in results)
        assert all(r[4]["info"]["cg_fused"] == 0 and r[4]["info"]["mg_cycles"] == r[0] for r in results)
        o = M.oracle(c, 1)  # the faces (boundary values) are set once and never written
        P = o.P.copy()
        P[2:-2, 2:-2, 2:-2] = Gf[2:-2, 2:-2, 2:-2]
        return dict(itr=results[0][0], hist=list(results[0][2]), P=P, info=results[0][4]["info"])

    g = _check(c, run)
    assert g["info"]["mg_levels"] == len(D.mg_level_dims(c["gsz"]))


def test_pcg_mg_two_rccl_ranks_equal_single_domain():
    """two processes over RCCL, division (2, 1, 1), FP32: field and history byte-equal to the single-domain run"""
    from test_gpu_rccl import run_ranks, single
    c = next(c for c in PCG_CASES if c["prec"] == "f32")
    itr1, res1, hist1, P1 = single("f32", c["gsz"], "pcg", c["K"], c["coef"], "mg")
    recs, Gf, logs = run_ranks("f32", c["gsz"], "pcg", c["K"], c["coef"], (2, 1, 1), pc="mg")
    assert Gf[2:-2, 2:-2, 2:-2].tobytes() == P1[2:-2, 2:-2, 2:-2].tobytes()
    for rec in recs:
        info = rec["info"]
        assert info["rccl_ranks"] == 2 and info["mg_levels"] == len(D.mg_level_dims(c["gsz"])) and info["mg_gather_level"] > 0, info
        assert rec["itr"] == itr1 == c["K"] and rec["history"] == list(hist1)


@pytest.mark.parametrize("n,div", [(64, (2, 2, 2)), (128, (2, 1, 1))], ids=["64_2x2x2", "128_2x1x1"])
def test_decomposed_pcg_mg_f64_to_convergence(n, div):
    """the whole solve takes the oracle's iteration count"""
    from test_gpu_decomp import _decomposed
    o = M.run((n, n, n), 1000, 0.8, prec="f64")
    assert o.itr == (8 if n == 64 else 9)
    results, _ = _decomposed("f64", (n, n, n), "pcg", 1000, 0.8, div, "mg")
    for itr, res, hist, P, loc in results:
        assert itr == o.itr, (itr, o.itr)
        assert loc["info"]["mg_cycles"] == itr
        ok, worst = _f64_close(hist, [v for _, v in o.history], [1e-9 * v for _, v in o.history])
        assert ok, worst
