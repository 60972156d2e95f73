"""The red-black V-cycle preconditioner of `pcg ... mgrb` on the GPU (-m gpu): the colour-sweep kernel alone, the LDS tail and the whole
cycle against the numpy restatement of tests/mgrb_parity.py, bit for bit in both precisions; level 0 through every pass that can run it;
PCG with it iteration by iteration against the exact-dot oracle (bars of tests/test_gpu_pcg.py); solves to convergence; an `mg` handle beside
an `mgrb` one; the command line and its refusals."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_parity as M  # noqa: E402
import mgrb_parity as RB  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402
from test_gpu_mg import SHAPES, _cli, _hip, _level_array, _put, _rand  # noqa: E402
from test_gpu_pcg import _check, _f64_close  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OMG = 1.2
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _inner_equal(dev, sz, idx, ref, what):
    got = dev.get()
    assert got[M.inner(sz, idx)].tobytes() == ref.tobytes(), what
    full = np.zeros_like(got)
    full[M.inner(sz, idx)] = ref
    assert got.tobytes() == full.tobytes(), what + ": wrote outside the level's box"


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", SHAPES, ids=IDS)
def test_colour_sweep_and_tail_bit_for_bit(gsz, prec):
    """mg_rb_k: both colours from an iterate, and the two colours of an iteration from zero in either order over an array full of other
    numbers (which must not be read), at every level >= 1; the tail from every level that fits"""
    hip = _hip(prec)
    R = hip.real
    rng = np.random.default_rng(7)
    idx0, _ = O.range_inner_index(list(gsz), [-1] * 6)
    n0 = M.n0_of(idx0)
    dims = M.level_dims(n0)
    arrays = []
    tails = 0
    try:
        for l, n in enumerate(dims):
            if l == 0:
                continue
            sz, idx = _level_array(n)
            shape = (n[1], n[0], n[2])
            u, b = _rand(rng, shape, R), _rand(rng, shape, R)
            db = _put(hip, sz, idx, b)
            arrays.append(db)
            for c in (0, 1):
                dx = _put(hip, sz, idx, u)
                arrays.append(dx)
                assert hip.mg_rb(dx, db, sz, idx, l, n0, OMG, c)
                _inner_equal(dx, sz, idx, RB.sweep(u, b, l, n0, OMG, c), f"level {l} colour {c} from u")
                # from zero: first colour c, then the other one, over u's numbers
                dx = _put(hip, sz, idx, u)
                arrays.append(dx)
                assert hip.mg_rb(dx, db, sz, idx, l, n0, OMG, c, zero=1)
                first = RB.sweep(None, b, l, n0, OMG, c)
                assert np.array_equal(dx.get()[M.inner(sz, idx)][RB.colour(shape) == c], first[RB.colour(shape) == c]), f"level {l} colour {c} from zero"
                assert hip.mg_rb(dx, db, sz, idx, l, n0, OMG, 1 - c, zero=2)
                _inner_equal(dx, sz, idx, RB.sweep(first, b, l, n0, OMG, 1 - c), f"level {l} colours {c}, {1 - c} from zero")
            dx = _put(hip, sz, idx, u)
            arrays.append(dx)
            if hip.mg_tail_rb(dx, db, sz, idx, l, n0, OMG):
                tails += 1
                _inner_equal(dx, sz, idx, RB.vcycle(b, l, n0, R(OMG)), f"tail from level {l}")
        assert tails >= 1
        # refused: level 0 (it runs the red-black passes), a level that does not match n0, a colour that is none
        sz, idx = _level_array(dims[-1])
        assert not hip.mg_rb(arrays[1], arrays[0], list(gsz), idx0, 0, n0, OMG, 0)
        assert not hip.mg_rb(arrays[-1], db, sz, idx, len(dims) - 1, n0, OMG, 2)
        szw, idxw = _level_array(tuple(v + 1 for v in dims[-1]))
        assert not hip.mg_rb(arrays[-1], db, szw, idxw, len(dims) - 1, n0, OMG, 0)
    finally:
        hip.sync()
        for a in arrays:
            a.free()


def _apply_gpu(prec, gsz, r_inner, monkeypatch, tail=1, rb4=None, zero4=None, omg=OMG, create="mg_create_rb"):
    monkeypatch.setenv("CZ_MG_TAIL", str(tail))
    if zero4 is not None:
        monkeypatch.setenv("CZ_MGRB_ZERO4", str(zero4))
    hip = _hip(prec)
    idx, _ = O.range_inner_index(list(gsz), [-1] * 6)
    sz = list(gsz)
    if rb4 is not None:
        hip.lib.czhip_set_rb4(rb4, -1, -1)
    h = getattr(hip, create)(sz, idx)
    assert h
    dr, dz = _put(hip, sz, idx, r_inner), _put(hip, sz, idx, None)
    try:
        assert hip.mg_kind(h) == (2 if create == "mg_create_rb" else 1)
        levels = hip.mg_levels(h)
        assert hip.mg_apply(h, dz, dr, omg)
        z1 = dz.get()
        assert hip.mg_apply(h, dz, dr, omg)  # a second application over the first one's z: the same bits (z is not read)
        assert dz.get().tobytes() == z1.tobytes()
        return z1, levels
    finally:
        hip.sync()
        hip.lib.czhip_set_rb4(1, -1, -1)
        hip.mg_destroy(h)
        dr.free(), dz.free()


def _rhs(prec, gsz, seed=11):
    k = O.Kernels("oracle", prec)
    idx, _ = O.range_inner_index(list(gsz), [-1] * 6)
    r = k.alloc(gsz)
    ins = M.inner(gsz, idx)
    r[ins] = _rand(np.random.default_rng(seed), r[ins].shape, k.real)
    return k, idx, r, ins


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", SHAPES + [(6, 6, 6)], ids=IDS + ["6x6x6"])
def test_apply_equals_restated_vcycle(gsz, prec, monkeypatch):
    """czhip_mg_apply_async on an mgrb handle against the restated cycle (level 0 through the oracle's psor2sma_core), CZ_MG_TAIL 1 and 0 the
    same bits; 6^3: level 0 is the coarsest"""
    k, idx, r, ins = _rhs(prec, gsz)
    ref = RB.apply(k, r, list(gsz), idx, OMG)
    z1, levels = _apply_gpu(prec, gsz, r[ins], monkeypatch, 1)
    assert levels == len(M.level_dims(M.n0_of(idx)))
    assert z1.tobytes() == ref.tobytes(), f"V-cycle differs from the restatement ({levels} levels)"
    z0, _ = _apply_gpu(prec, gsz, r[ins], monkeypatch, 0)
    assert z0.tobytes() == z1.tobytes(), "CZ_MG_TAIL=0 changed the bits"


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", [(33, 47, 61), (64, 64, 64), (6, 6, 6), (40, 40, 1100)], ids=["33x47x61", "64x64x64", "6x6x6", "40x40x1100"])
def test_level0_through_every_pass_gives_equal_bits(gsz, prec, monkeypatch):
    """level 0 by the two-iteration pass rb4_k (forced also on small grids), by single red-black passes (rb4 off), and with the first two
    iterations as rb4_k over a cleared array (CZ_MGRB_ZERO4=1): the restatement's bits every time"""
    k, idx, r, ins = _rhs(prec, gsz, 13)
    ref = RB.apply(k, r, list(gsz), idx, OMG).tobytes()
    for rb4, zero4 in ((0, 0), (2, 0), (2, 1), (1, 1)):
        z, _ = _apply_gpu(prec, gsz, r[ins], monkeypatch, rb4=rb4, zero4=zero4)
        assert z.tobytes() == ref, f"rb4 {rb4}, CZ_MGRB_ZERO4 {zero4}"


def test_create_refuses_other_coefficients():
    hip = _hip("f64")
    idx, _ = O.range_inner_index([16, 16, 16], [-1] * 6)
    assert not hip.mg_create_rb([16, 16, 16], idx, cf=(1, 1, 1, 1, 1, 2, 7))
    assert not hip.mg_create_rb([16, 16, 16], idx, cf=(1, 1, 1, 1, 1, 1, 5))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_mg_and_mgrb_handles_alive_together(prec, monkeypatch):
    """both kinds of handle at once, applied in turn: each gives its own restatement's bits"""
    gsz = (33, 47, 61)
    k, idx, r, ins = _rhs(prec, gsz, 17)
    hip = _hip(prec)
    sz = list(gsz)
    hj, hr = hip.mg_create(sz, idx), hip.mg_create_rb(sz, idx)
    assert hj and hr and hip.mg_kind(hj) == 1 and hip.mg_kind(hr) == 2 and hip.mg_kind(None) == 0
    dr, dz = _put(hip, sz, idx, r[ins]), _put(hip, sz, idx, None)
    try:
        ref_j, ref_r = M.apply(k, r, sz, idx, 0.8).tobytes(), RB.apply(k, r, sz, idx, 0.8).tobytes()
        for _ in range(2):
            assert hip.mg_apply(hj, dz, dr, 0.8)
            assert dz.get().tobytes() == ref_j, "mg beside an mgrb handle"
            assert hip.mg_apply(hr, dz, dr, 0.8)
            assert dz.get().tobytes() == ref_r, "mgrb beside an mg handle"
    finally:
        hip.sync()
        hip.mg_destroy(hj), hip.mg_destroy(hr)
        dr.free(), dz.free()


def _levels(c):
    return len(M.level_dims(M.n0_of(O.range_inner_index(list(c["gsz"]), [-1] * 6)[0])))


def _patch(monkeypatch):
    import test_gpu_pcg as TP
    monkeypatch.setattr(TP.CP, "oracle", RB.oracle)
    monkeypatch.setattr(TP.CP, "envelope_f64", RB.envelope_f64)
    monkeypatch.setattr(TP.CP, "premise_f32", lambda c, o, perturbed=False: RB.premise_f32(c, o))


@pytest.mark.parametrize("c", RB.CASES, ids=[c["id"] for c in RB.CASES])
def test_pcg_mgrb_iterations_vs_exact_dot_oracle(c, monkeypatch):
    """FP32: field, history and count bit for bit; FP64: within 2 E + 8 ulp (tests/test_gpu_pcg.py's bars)"""
    _patch(monkeypatch)
    g = _check(c)
    assert g["info"]["mg_cycles"] == c["K"] and g["info"]["mg_levels"] == _levels(c) and g["info"]["mg_smoother"] == 2
    assert g["info"]["cg_fused"] == c["K"]


@pytest.mark.parametrize("c", [c for c in RB.CASES if c["gsz"] in ((33, 47, 61), (64, 64, 64))], ids=lambda c: c["id"])
def test_pcg_mgrb_unfused_vs_exact_dot_oracle(c, monkeypatch):
    """CZ_CG_FUSE=0: the separate update, SpMV and dot launches, against the same oracle"""
    _patch(monkeypatch)
    monkeypatch.setenv("CZ_CG_FUSE", "0")
    g = _check(c)
    assert g["info"]["cg_fused"] == 0 and g["info"]["mg_cycles"] == c["K"]


@pytest.mark.parametrize("omg", [0.8, 1.2])
@pytest.mark.parametrize("n", [64, 128])
def test_pcg_mgrb_f64_to_convergence(n, omg):
    """the whole solve: the count equals the oracle's (every perturbed run agrees) and lies below mg's, error_max within the perturbed runs'
    envelope"""
    from cubez_amd import CZ
    gsz = (n, n, n)
    r = {p: RB.run(gsz, 1000, omg, prec="f64", perturb=p, with_error=True) for p in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr
    assert r[0].itr <= 8  # (mg at 0.8: 8 at 64^3, 9 at 128^3)
    cz = CZ("f64", quiet=True)
    try:
        assert cz.setup([n, n, n, "pcg", 1000, omg, "mgrb"]) == 1
        itr = cz.solve()
        info = cz.info()
        err, _ = cz.error_max()
    finally:
        cz.close()
    assert itr == r[0].itr, (itr, r[0].itr)
    assert info["mg_cycles"] == itr and info["mg_levels"] == len(M.level_dims((n - 2,) * 3)) and info["mg_smoother"] == 2
    E = max(abs(r[1].errmax - r[0].errmax), abs(r[-1].errmax - r[0].errmax))
    ok, worst = _f64_close([err], [r[0].errmax], [E])
    assert ok, (err, r[0].errmax, E, worst)


def test_precondition_applies_the_cycle():
    """cz_precondition of a driver set up with mgrb is the restated cycle"""
    from cubez_amd import CZ
    gsz = (33, 47, 61)
    k, idx, r, ins = _rhs("f64", gsz, 19)
    cz = CZ("f64", quiet=True)
    try:
        assert cz.setup(list(gsz) + ["pcg", 1, 1.0, "mgrb"]) == 1
        z = cz.precondition(r)
    finally:
        cz.close()
    assert z.tobytes() == RB.apply(k, r, list(gsz), idx, 1.0).tobytes()


def test_cli_pcg_mgrb(tmp_path):
    p = _cli("f64", [128, 128, 128, "pcg", 1000, 1.2, "mgrb"], tmp_path)
    assert p.returncode == 0, p.stderr
    assert "Preconditioner = MGRB" in p.stdout
    o = RB.run((128, 128, 128), 1000, 1.2, prec="f64")
    assert f"Iter = {o.itr} " in p.stdout, p.stdout[-400:]
    assert (tmp_path / "pcg.txt").exists()
    assert len((tmp_path / "pcg.txt").read_text().splitlines()) == o.itr + 1


def test_cli_pcg_mgrb_refusals(tmp_path):
    """a coefficient outside (0, 1.2] is refused with one line and exit status 0, before any solve"""
    for coef in (1.3, 0.0, -0.5):
        p = _cli("f64", [32, 32, 32, "pcg", 100, coef, "mgrb"], tmp_path)
        assert p.returncode == 0 and "Invalid coefficient for pcg with mgrb" in p.stdout and "Iter =" not in p.stdout, p.stdout
    p = _cli("f64", [32, 32, 32, "pcg", 100, 0.8, "mgrbx"], tmp_path)
    assert p.returncode == 0 and "Invalid preconditioner for pcg" in p.stdout and "Iter =" not in p.stdout, p.stdout


def test_two_ranks_are_refused(tmp_path):
    """mgrb on more than one rank (LOCAL transport, two ranks as threads of a child process): one line, exit status 0, no solve"""
    child = textwrap.dedent(f"""
        import ctypes as C, sys, threading
        sys.path.insert(0, {ROOT!r})
        from cubez_amd import CZ, load
        lib = load("f64")
        lib.cz_comm_local_world.restype = C.c_void_p
        lib.cz_comm_bootstrap_local.argtypes = [C.c_void_p, C.c_int]
        world = lib.cz_comm_local_world(2)
        def work(q):
            lib.cz_comm_bootstrap_local(world, q)
            cz = CZ("f64", quiet=False)
            cz.setup([32, 32, 32, "pcg", 10, 0.8, "mgrb", 2, 1, 1])
            print("SET UP", flush=True)
        th = [threading.Thread(target=work, args=(q,)) for q in range(2)]
        [t.start() for t in th]
        [t.join(timeout=60) for t in th]
        print("NOT REFUSED", flush=True)
        """)
    p = subprocess.run([sys.executable, "-c", child], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr[-600:])
    assert "pcg with mgrb runs on a single domain only (2 ranks)" in p.stdout, p.stdout
    assert "SET UP" not in p.stdout and "NOT REFUSED" not in p.stdout and "Iter =" not in p.stdout, p.stdout
