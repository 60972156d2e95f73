"""The multigrid V-cycle preconditioner of `pcg ... mg` on the GPU (-m gpu): each level kernel alone and the whole cycle against the numpy
restatement of tests/mg_parity.py, bit for bit in both precisions; PCG with it iteration by iteration against the exact-dot oracle (bars of
tests/test_gpu_pcg.py); solves to convergence; the command line and its refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_parity as M  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402
from test_gpu_pcg import _check, _f64_close  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(9, 7, 12), (33, 47, 61), (64, 64, 64), (40, 40, 1100), (3, 40, 40)]  # (3, 40, 40): a unit extent (one inner point in i)
OMG = 0.8


def _hip(prec):
    from cubez_amd.lib import CzHip
    return CzHip(prec)


def _level_array(n):
    """the hierarchy's layout of a level of n = (ni, nj, nk) points: sz = n + 2, inner box 2 .. n + 1"""
    sz = [v + 2 for v in n]
    idx = [2, n[0] + 1, 2, n[1] + 1, 2, n[2] + 1]
    return sz, idx


def _put(hip, sz, idx, inner_vals):
    R = hip.real
    host = np.zeros((sz[1] + 4, sz[0] + 4, sz[2] + 4), dtype=R)
    if inner_vals is not None:
        host[M.inner(sz, idx)] = inner_vals
    return hip.alloc(sz, host)


def _rand(rng, shape, R):
    return rng.standard_normal(shape).astype(R)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_level_kernels_bit_for_bit(gsz, prec):
    """smooth (from zero and from u), restrict and prolong at every level of the box against the restatement"""
    hip = _hip(prec)
    R = hip.real
    rng = np.random.default_rng(7)
    idx0, _ = O.range_inner_index(list(gsz), [-1] * 6)
    n0 = M.n0_of(idx0)
    dims = M.level_dims(n0)
    arrays = []
    try:
        for l, n in enumerate(dims):
            sz, idx = _level_array(n)
            shape = (n[1], n[0], n[2])
            u, b = _rand(rng, shape, R), _rand(rng, shape, R)
            du, db, dw = _put(hip, sz, idx, u), _put(hip, sz, idx, b), _put(hip, sz, idx, None)
            arrays += [du, db, dw]
            for src, ref in ((None, M.smooth(None, b, l, n0, OMG)), (du, M.smooth(u, b, l, n0, OMG))):
                assert hip.mg_smooth(src, dw, db, sz, idx, l, n0, OMG)
                got = dw.get()
                assert got[M.inner(sz, idx)].tobytes() == ref.tobytes(), f"smooth level {l} {'from u' if src else 'from zero'}"
                ref_full = np.zeros_like(got)
                ref_full[M.inner(sz, idx)] = ref
                assert got.tobytes() == ref_full.tobytes(), "smooth wrote outside the level's box"
            if l + 1 < len(dims):
                szc, idxc = _level_array(dims[l + 1])
                dbc = _put(hip, szc, idxc, None)
                arrays.append(dbc)
                assert hip.mg_restrict(dbc, szc, idxc, du, db, sz, idx, l, n0)
                assert dbc.get()[M.inner(szc, idxc)].tobytes() == M.restrict(u, b, l, n0).tobytes(), f"restrict level {l}"
                xc = _rand(rng, (dims[l + 1][1], dims[l + 1][0], dims[l + 1][2]), R)
                dxc = _put(hip, szc, idxc, xc)
                arrays.append(dxc)
                assert hip.mg_prolong(dw, du, dxc, szc, idxc, sz, idx, l, n0)
                assert dw.get()[M.inner(sz, idx)].tobytes() == M.prolong(u, xc).tobytes(), f"prolong level {l}"
                # in place (u = x)
                assert hip.mg_prolong(du, du, dxc, szc, idxc, sz, idx, l, n0)
                assert du.get()[M.inner(sz, idx)].tobytes() == M.prolong(u, xc).tobytes(), f"prolong level {l} in place"
            # the tail from this level (where its levels fit the LDS) is the restated cycle
            dx = _put(hip, sz, idx, None)
            arrays.append(dx)
            if l > 0 and hip.mg_tail(dx, db, sz, idx, l, n0, OMG):
                assert dx.get()[M.inner(sz, idx)].tobytes() == M.vcycle(b, l, n0, OMG).tobytes(), f"tail from level {l}"
        # a level that does not match n0 is refused
        sz, idx = _level_array(tuple(v + 1 for v in dims[-1]))
        assert not hip.mg_smooth(None, arrays[2], arrays[1], sz, idx, len(dims) - 1, n0, OMG)
    finally:
        hip.sync()
        for a in arrays:
            a.free()


def _apply_gpu(prec, gsz, r_inner, monkeypatch, tail):
    monkeypatch.setenv("CZ_MG_TAIL", str(tail))
    hip = _hip(prec)
    idx, _ = O.range_inner_index(list(gsz), [-1] * 6)
    sz = list(gsz)
    h = hip.mg_create(sz, idx)
    assert h
    dr, dz = _put(hip, sz, idx, r_inner), _put(hip, sz, idx, None)
    try:
        levels = hip.mg_levels(h)
        assert hip.mg_apply(h, dz, dr, OMG)
        z1 = dz.get()
        assert hip.mg_apply(h, dz, dr, OMG)  # a second application over the first one's z: the same bits (z is not read)
        assert dz.get().tobytes() == z1.tobytes()
        return z1, levels
    finally:
        hip.sync()
        hip.mg_destroy(h)
        dr.free(), dz.free()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", SHAPES + [(6, 6, 6)], ids=["x".join(map(str, s)) for s in SHAPES + [(6, 6, 6)]])
def test_apply_equals_restated_vcycle(gsz, prec, monkeypatch):
    """czhip_mg_apply_async against the restated V-cycle (level 0 through the oracle's jacobi), CZ_MG_TAIL 1 and 0 the same bits"""
    k = O.Kernels("oracle", prec)
    idx, _ = O.range_inner_index(list(gsz), [-1] * 6)
    rng = np.random.default_rng(11)
    r = k.alloc(gsz)
    ins = M.inner(gsz, idx)
    r[ins] = _rand(rng, r[ins].shape, k.real)
    ref = M.apply(k, r, list(gsz), idx, OMG)
    z1, levels = _apply_gpu(prec, gsz, r[ins], monkeypatch, 1)
    assert levels == len(M.level_dims(M.n0_of(idx)))
    assert z1.tobytes() == ref.tobytes(), f"V-cycle differs from the restatement ({levels} levels)"
    z0, _ = _apply_gpu(prec, gsz, r[ins], monkeypatch, 0)
    assert z0.tobytes() == z1.tobytes(), "CZ_MG_TAIL=0 changed the bits"


def test_create_refuses_other_coefficients():
    hip = _hip("f64")
    idx, _ = O.range_inner_index([16, 16, 16], [-1] * 6)
    assert not hip.mg_create([16, 16, 16], idx, cf=(1, 1, 1, 1, 1, 2, 7))
    assert not hip.mg_create([16, 16, 16], idx, cf=(1, 1, 1, 1, 1, 1, 5))


@pytest.mark.parametrize("c", M.CASES, ids=[c["id"] for c in M.CASES])
def test_pcg_mg_iterations_vs_exact_dot_oracle(c, monkeypatch):
    """FP32: field, history and count bit for bit; FP64: within 2 E + 8 ulp (tests/test_gpu_pcg.py's bars)"""
    import test_gpu_pcg as TP
    monkeypatch.setattr(TP.CP, "oracle", M.oracle)
    monkeypatch.setattr(TP.CP, "envelope_f64", M.envelope_f64)
    monkeypatch.setattr(TP.CP, "premise_f32", lambda c, o, perturbed=False: M.premise_f32(c, o))
    g = _check(c)
    assert g["info"]["mg_cycles"] == c["K"] and g["info"]["mg_levels"] == len(M.level_dims(M.n0_of(O.range_inner_index(list(c["gsz"]), [-1] * 6)[0])))


@pytest.mark.parametrize("n", [64, 128])
def test_pcg_mg_f64_to_convergence(n):
    """the whole solve: the count equals the oracle's (every perturbed run agrees), error_max within the perturbed runs' envelope"""
    from cubez_amd import CZ
    gsz = (n, n, n)
    r = {p: M.run(gsz, 1000, 0.8, prec="f64", perturb=p, with_error=True) for p in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr
    assert r[0].itr <= (10 if n == 64 else 12)
    cz = CZ("f64", quiet=True)
    try:
        assert cz.setup([n, n, n, "pcg", 1000, 0.8, "mg"]) == 1
        itr = cz.solve()
        info = cz.info()
        err, _ = cz.error_max()
    finally:
        cz.close()
    assert itr == r[0].itr, (itr, r[0].itr)
    assert info["mg_cycles"] == itr and info["mg_levels"] == len(M.level_dims((n - 2,) * 3))
    E = max(abs(r[1].errmax - r[0].errmax), abs(r[-1].errmax - r[0].errmax))
    ok, worst = _f64_close([err], [r[0].errmax], [E])
    assert ok, (err, r[0].errmax, E, worst)


def _cli(prec, args, cwd):
    exe = os.path.join(ROOT, "cubez_amd", f"cz_{prec}")
    return subprocess.run([exe] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


def test_cli_pcg_mg(tmp_path):
    p = _cli("f64", [128, 128, 128, "pcg", 1000, 0.8, "mg"], tmp_path)
    assert p.returncode == 0, p.stderr
    assert "Preconditioner = MG" in p.stdout
    o = M.run((128, 128, 128), 1000, 0.8, prec="f64")
    assert f"Iter = {o.itr} " in p.stdout, p.stdout[-400:]
    assert (tmp_path / "pcg.txt").exists()
    assert len((tmp_path / "pcg.txt").read_text().splitlines()) == o.itr + 1


def test_cli_pcg_mg_refusals(tmp_path):
    """a coefficient outside (0, 1] is refused with one line and exit status 0, before any solve (the refusal of decomposed runs is the same
    kind of line in CZ::setLS; a test of it would need two ranks that each end their process)"""
    p = _cli("f64", [32, 32, 32, "pcg", 100, 1.2, "mg"], tmp_path)
    assert p.returncode == 0 and "Invalid coefficient for pcg with mg" in p.stdout and "Iter =" not in p.stdout, p.stdout
    p = _cli("f64", [32, 32, 32, "pcg", 100, 0.0, "mg"], tmp_path)
    assert p.returncode == 0 and "Invalid coefficient for pcg with mg" in p.stdout and "Iter =" not in p.stdout, p.stdout
