"""Mixed-precision refinement on the GPU (-m gpu): cz_get_residual and cz_add_field byte for byte against their numpy
restatement on the oracle's blas_calc_rk_ (tests/refine_parity.py), the sum of squares within the order-free bound of a double sum, decomposed
runs on the LOCAL transport, the refusals, cubez_amd.Refined against the CPU restatement of its loop, and the stream hand-over.

The sum: N non-negative double terms summed in any order lie within (N + 1) 2^-52 relative of their correctly rounded sum (refine_parity.sum_bound
derives it); the squares themselves are exact products of the bytes that were compared, rounded once each."""
import ctypes as C
import functools
import math
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import problem_parity as PP  # noqa: E402
import refine_parity as RP  # noqa: E402
from test_gpu_problem import FORM, _handle, _layouts, _real, _torch  # noqa: E402

pytestmark = pytest.mark.gpu
SCALES = [1.0, 2.0 ** -7, 2.0 ** 9]
WIDTHS = [np.float32, np.float64]
SENTINEL = -77.0


@functools.lru_cache(maxsize=None)
def _problem(gsz, prec):
    """(b, p, r, fsum of r^2): a seeded problem in the handle's precision and the restated residual of it"""
    b, p = PP.problem(gsz, prec, 11)
    r = RP.residual(p, b, prec)
    for ax in range(3):  # Dirichlet faces are 0
        assert not r.take([0, -1], axis=ax).any()
    return b, p, r, RP.sumsq(r)


def _inner_view(want, base_shape, name, gsz):
    ni, nj, nk = gsz
    return (want.transpose(2, 1, 0) if name == "fortran" else want.transpose(2, 0, 1) if name == "perm_jki" else want.transpose(0, 2, 1) if name == "perm_ikj"
            else want[2:2 + ni, 1:1 + nj, 3:3 + nk] if name == "slice" else want[:, :, ::2] if name == "every_other" else want)


def _tdt(torch, T):
    return torch.float32 if T == np.float32 else torch.float64


def _check_residual(cz, gsz, prec, where, force, names=None):
    b, p, r, exact = _problem(gsz, prec)
    cz.set_rhs(b)
    cz.set_field(p)
    n = int(np.prod(gsz))
    sums = []
    for T in WIDTHS:
        if where == "device":
            torch = _torch()
            lay = _layouts(torch, gsz, _tdt(torch, T), device="cuda")
        else:
            lay = _layouts(np, gsz, T)
        for name, (base, view) in lay.items():
            if names and name not in names:
                continue
            for scale in SCALES:
                if where == "device":
                    base.fill_(SENTINEL)
                else:
                    base[...] = SENTINEL
                out, ss = cz.get_residual(out=view, scale=scale)
                assert cz.info()["field_form"] == (3 if force else FORM[name]), (name, cz.info()["field_form"])
                got = base.cpu().numpy() if where == "device" else base
                want = np.full(got.shape, SENTINEL, dtype=T)
                _inner_view(want, got.shape, name, gsz)[...] = RP.scaled(r, scale, T)
                assert got.tobytes() == want.tobytes(), f"{name} {np.dtype(T).name} scale {scale}: the residual differs from the restatement"
                print(f"{gsz} {prec} {name} {np.dtype(T).name} {scale}: sumsq {ss!r} exact {exact!r} rel {abs(ss - exact) / exact:.3g} bound {RP.sum_bound(n):.3g}")
                assert abs(ss - exact) <= RP.sum_bound(n) * exact
                sums.append(ss)
    assert len(set(np.float64(s).tobytes() for s in sums)) == 1, "the sum of squares depends on the destination or the call"
    return sums[0]


# (9, 7, 12), (33, 47, 61): the issue's boxes; (5, 5, 3): a k row shorter than one destination vector; (12, 9, 7): a k extent that is no multiple
# of either vector width -- the smallest shapes at which the ragged ends of a row can go wrong
@pytest.mark.parametrize("force", [0, 3], ids=["form_by_strides", "generic_forced"])
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", [(9, 7, 12), (33, 47, 61), (5, 5, 3), (12, 9, 7)], ids=lambda g: "x".join(map(str, g)))
def test_residual_byte_for_byte(gsz, prec, where, force, monkeypatch):
    """every layout, both destination widths, three scales, host and device, the form the strides choose and the generic one forced: the bytes of
    the restatement (the two forms therefore give equal bytes), nothing but the brick written, Dirichlet faces 0, the sum within the bound and
    the same bits from every call"""
    if force:
        monkeypatch.setenv("CZ_FIELD_FORM", str(force))
    cz = _handle(prec, list(gsz) + ["jacobi", 10, 0.8])
    try:
        _check_residual(cz, gsz, prec, where, force)
    finally:
        cz.close()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", [(9, 7, 12), (33, 47, 61)], ids=lambda g: "x".join(map(str, g)))
def test_norm_only_gives_the_same_bits(gsz, prec):
    b, p, r, exact = _problem(gsz, prec)
    cz = _handle(prec, list(gsz) + ["jacobi", 10, 0.8])
    try:
        cz.set_rhs(b)
        cz.set_field(p)
        none, s0 = cz.get_residual()
        assert none is None
        out, s1 = cz.get_residual(dtype=np.float32)
        assert out.tobytes() == RP.scaled(r, 1.0, np.float32).tobytes()
        _, s2 = cz.get_residual(out=np.asfortranarray(np.zeros(gsz)), scale=4.0)
        _, s3 = cz.get_residual()
        assert np.float64(s0).tobytes() == np.float64(s1).tobytes() == np.float64(s2).tobytes() == np.float64(s3).tobytes()
        assert abs(s0 - exact) <= RP.sum_bound(int(np.prod(gsz))) * exact
        assert cz.get_field().tobytes() == p.tobytes()  # (the iterate is not touched)
    finally:
        cz.close()


@pytest.mark.parametrize("force", [0, 3], ids=["form_by_strides", "generic_forced"])
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", [(9, 7, 12), (33, 47, 61), (5, 5, 3), (12, 9, 7)], ids=lambda g: "x".join(map(str, g)))
def test_add_field_byte_for_byte(gsz, prec, where, force, monkeypatch):
    """P afterwards (cz_field: the whole padded array) = P + (REAL)e (REAL)scale on the updated cells, faces and guide cells untouched; both
    source widths, every layout, corrections accumulating from one call to the next"""
    R = _real(prec)
    if force:
        monkeypatch.setenv("CZ_FIELD_FORM", str(force))
    b, p, _, _ = _problem(gsz, prec)
    cz = _handle(prec, list(gsz) + ["jacobi", 10, 0.8])
    try:
        cz.set_field(p)
        before = cz.field()
        rng = np.random.default_rng(5)
        cur = p
        for T in WIDTHS:
            if where == "device":
                torch = _torch()
                lay = _layouts(torch, gsz, _tdt(torch, T), device="cuda")
            else:
                lay = _layouts(np, gsz, T)
            for (name, (base, view)), scale in zip(lay.items(), SCALES * 2):
                e = (rng.random(gsz) - 0.5).astype(T)
                if where == "device":
                    view.copy_(torch.from_numpy(e).cuda())
                else:
                    view[...] = e
                cz.add_field(view, scale)
                assert cz.info()["field_form"] == (3 if force else FORM[name]), (name, cz.info()["field_form"])
                cur = RP.add(cur, e, scale)
                assert cur.dtype == R
                assert cz.field().tobytes() == PP.pad(cur, into=before).tobytes(), f"{name} {np.dtype(T).name}: P differs from the restatement"
    finally:
        cz.close()


# ---- decomposed runs on the LOCAL transport (ranks as threads, as tests/test_gpu_decomp.py and tests/test_gpu_mg_decomp.py run them; their
# helpers are bound to their own workloads, so the thread frame is restated here for one or both libraries)
def _ranks(n, precs, work):
    from cubez_amd import load
    libs, worlds = {}, {}
    for prec in precs:
        lib = libs[prec] = load(prec)
        lib.cz_comm_local_world.restype = C.c_void_p
        lib.cz_comm_bootstrap_local.argtypes = [C.c_void_p, C.c_int]
        lib.cz_comm_local_world_free.argtypes = [C.c_void_p]
        worlds[prec] = lib.cz_comm_local_world(n)
    results, errors = [None] * n, []

    def run(q):
        try:
            for prec in precs:
                libs[prec].cz_comm_bootstrap_local(worlds[prec], q)
            results[q] = work(q)
        except BaseException as e:  # noqa: BLE001
            errors.append((q, repr(e)))

    th = [threading.Thread(target=run, args=(q,)) for q in range(n)]
    [t.start() for t in th]
    [t.join(timeout=90) for t in th]
    if any(t.is_alive() for t in th):  # a rank stuck in a collective cannot be unblocked
        sys.stderr.write(f"DEADLOCK: {n} ranks did not finish in 90 s\n")
        sys.stderr.flush()
        os._exit(3)
    assert not errors, errors
    for prec in precs:
        libs[prec].cz_comm_local_world_free(worlds[prec])
    return results


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("div", [(2, 1, 2), (2, 2, 2)], ids=lambda d: "x".join(map(str, d)))
def test_decomposed_equals_single_domain(div, prec):
    from cubez_amd import CZ
    gsz, scale, T = (21, 18, 23), 2.0 ** -7, np.float32 if prec == "f64" else np.float64
    b, p, r, exact = _problem(gsz, prec)
    e = (np.random.default_rng(9).random(gsz) - 0.5).astype(T)
    R1, R2, X = (np.full(gsz, np.nan, dtype=T), np.full(gsz, np.nan, dtype=T), np.full(gsz, np.nan, dtype=_real(prec)))

    def work(q):
        cz = CZ(prec, quiet=True)
        try:
            assert cz.setup(list(gsz) + ["jacobi", 10, 0.8] + list(div)) == 1
            sl = cz.global_slice()
            cz.set_rhs(b[sl])
            cz.set_field(p[sl])
            _, s1 = cz.get_residual(out=R1[sl], scale=scale)
            _, s1n = cz.get_residual()
            cz.add_field(e[sl], 0.5)
            cz.get_field(X[sl])
            _, s2 = cz.get_residual(out=R2[sl], scale=scale)  # (sees the neighbours' corrected cells: the ghost layers were refreshed)
            return s1, s1n, s2
        finally:
            cz.close()

    res = _ranks(div[0] * div[1] * div[2], [prec], work)
    assert all(np.array(q).tobytes() == np.array(res[0]).tobytes() for q in res), "the ranks disagree about the sum"
    s1, s1n, s2 = res[0]
    n = int(np.prod(gsz))
    assert np.float64(s1).tobytes() == np.float64(s1n).tobytes()
    assert abs(s1 - exact) <= RP.sum_bound(n) * exact
    assert R1.tobytes() == RP.scaled(r, scale, T).tobytes(), "the bricks' residuals differ from the single-domain one"
    x = RP.add(p, e, 0.5)
    assert X.tobytes() == x.tobytes()
    r2 = RP.residual(x, b, prec)
    assert R2.tobytes() == RP.scaled(r2, scale, T).tobytes(), "the residual after add_field did not see the neighbours' new values"
    assert abs(s2 - RP.sumsq(r2)) <= RP.sum_bound(n) * RP.sumsq(r2)


# ---- refusals
def test_refusals_return_0_and_change_nothing():
    from cubez_amd import CZ
    gsz = (9, 7, 12)
    b, p, r, _ = _problem(gsz, "f32")
    a = np.zeros(gsz, dtype=np.float32)
    st, ss = (C.c_longlong * 3)(84, 12, 1), C.c_double(-1.0)
    cz = CZ("f32", quiet=True)
    res = lambda *x: cz.lib.cz_get_residual(cz.h, *x)  # noqa: E731
    add = lambda *x: cz.lib.cz_add_field(cz.h, *x)     # noqa: E731
    try:
        assert res(a.ctypes.data, 4, st, 0, None, 1.0, C.byref(ss)) == 0 and add(a.ctypes.data, 4, st, 0, None, 1.0) == 0  # before cz_setup
        assert cz.setup(list(gsz) + ["jacobi", 10, 0.8]) == 1
        cz.set_rhs(b)
        cz.set_field(p)
        before = cz.field().tobytes()
        for bad in ([a.ctypes.data, 4, None, 0, None, 1.0], [a.ctypes.data, 4, (C.c_longlong * 3)(84, 0, 1), 0, None, 1.0],  # NULL strides, a stride < 1
                    [a.ctypes.data, 4, st, 1, None, 1.0],                                                                     # host memory as device memory
                    [a.ctypes.data, 2, st, 0, None, 1.0], [a.ctypes.data, 16, st, 0, None, 1.0], [a.ctypes.data, 0, st, 0, None, 1.0],  # byte sizes
                    [a.ctypes.data + 2, 4, st, 0, None, 1.0],                                                                 # not aligned
                    [a.ctypes.data, 4, st, 0, None, 0.0], [a.ctypes.data, 4, st, 0, None, -2.0], [a.ctypes.data, 4, st, 0, None, math.inf],
                    [a.ctypes.data, 4, st, 0, None, math.nan], [a.ctypes.data, 4, st, 0, None, 1e-60]):                        # scales (1e-60 is 0 in FP32)
            assert res(*bad, C.byref(ss)) == 0, bad
            assert add(*bad) == 0, bad
        assert add(None, 4, st, 0, None, 1.0) == 0                                                # NULL source
        assert res(a.ctypes.data, 4, (C.c_longlong * 3)(1, 1, 1), 0, None, 1.0, C.byref(ss)) == 0  # cells of the destination alias
        assert res(a.ctypes.data, 4, st, 0, None, 1.0, None) == 0                                 # nowhere to put the sum
        assert res(None, 0, None, 0, None, math.nan, C.byref(ss)) == 0                            # the norm alone takes a scale too
        assert ss.value == -1.0 and not a.any() and cz.field().tobytes() == before
        with pytest.raises(ValueError):
            cz.get_residual(out=np.zeros(gsz, dtype=np.int32))
        with pytest.raises(ValueError):
            cz.add_field(np.zeros((9, 7, 13), dtype=np.float64))
        out, _ = cz.get_residual(dtype=np.float64)  # the handle is usable
        assert out.tobytes() == RP.scaled(r, 1.0, np.float64).tobytes() and cz.field().tobytes() == before
    finally:
        cz.close()
    maf = _handle("f32", list(gsz) + ["jacobi_maf", 10, 0.8])
    try:
        before = maf.field().tobytes()
        assert maf.lib.cz_get_residual(maf.h, a.ctypes.data, 4, st, 0, None, 1.0, C.byref(ss)) == 0
        assert maf.lib.cz_get_residual(maf.h, None, 0, None, 0, None, 1.0, C.byref(ss)) == 0
        assert maf.lib.cz_add_field(maf.h, a.ctypes.data, 4, st, 0, None, 1.0) == 0
        assert maf.field().tobytes() == before and ss.value == -1.0
    finally:
        maf.close()


# ---- Refined
@functools.lru_cache(maxsize=None)
def _restated(gsz):
    u, b, p = PP.manufactured(gsz)
    k, hist, x, ratios = RP.refine(b, p)
    assert k > 0 and RP.premise(ratios, 1e-10, int(np.prod([n - 2 for n in gsz])))  # (tests/test_refine_oracle.py shows both on the CPU)
    return b, p, k, hist


def _true_rel(b, p0, x):
    """|b - A x| / |b - A p0| and |b - A x| by a fresh FP64 handle"""
    cz = _handle("f64", list(b.shape) + ["jacobi", 1, 0.8])
    try:
        cz.set_rhs(b)
        cz.set_field(p0)
        _, s0 = cz.get_residual()
        cz.set_field(x)
        _, s = cz.get_residual()
        return math.sqrt(s) / math.sqrt(s0), math.sqrt(s)
    finally:
        cz.close()


@pytest.mark.parametrize("gsz", [(33, 47, 61), (64, 64, 64)], ids=lambda g: "x".join(map(str, g)))
def test_refined_follows_the_restated_loop(gsz):
    from cubez_amd import Refined
    torch = _torch()
    b, p, k, hist = _restated(gsz)
    rf = Refined(gsz)
    try:
        rf.set_rhs(torch.from_numpy(b).cuda())
        rf.set_field(p)
        steps = rf.solve()
        print("Refined", gsz, "outer", steps, "history", rf.history, "restated", hist)
        assert steps == k and [h[2] for h in rf.history] == [h[2] for h in hist] and [h[0] for h in rf.history] == list(range(1, k + 1))
        # (the ratios are FP64 quantities of iterates that agree to FP64 rounding of each correction, not bit for bit: a loose sanity bar only)
        assert np.allclose([h[1] for h in rf.history], [h[1] for h in hist], rtol=0.5)
        x = rf.get_field()
    finally:
        rf.close()
    rel, r1 = _true_rel(b, p, x)
    print("true relative residual", rel)
    assert rel <= 1e-10
    # the FP64 library alone, tightened to the same bar
    cz = _handle("f64", list(gsz) + ["pcg", 1000, 1.2, "mgrb"])
    try:
        cz.set_rhs(b)
        cz.set_field(p)
        _, s0 = cz.get_residual()
        eps = 1e-7
        while True:
            cz.set_eps(eps)
            assert cz.solve() > 0
            _, s = cz.get_residual()
            if math.sqrt(s) <= 1e-10 * math.sqrt(s0):
                break
            eps *= 0.1
            assert eps > 1e-16
        x64, r2 = cz.get_field(), math.sqrt(s)
    finally:
        cz.close()
    d = float(np.linalg.norm((x - x64).ravel()))
    print("|x_refined - x_fp64|", d, "bound", (r1 + r2) / RP.lambda_min(gsz))
    assert d <= (r1 + r2) / RP.lambda_min(gsz)


def test_refined_decomposed_takes_the_single_domain_counts():
    """pcg ... mg as the inner solver (mgrb runs on a single domain only): division (2, 1, 2) on the LOCAL transport, both libraries decomposed"""
    from cubez_amd import Refined
    torch = _torch()
    gsz, div, inner = (33, 47, 61), (2, 1, 2), ("pcg", 1000, 0.8, "mg")
    u, b, p = PP.manufactured(gsz)
    rf = Refined(gsz, inner=inner)
    try:
        rf.set_rhs(b)
        rf.set_field(p)
        steps, hist = rf.solve(), list(rf.history)
    finally:
        rf.close()
    assert steps > 0
    X = np.full(gsz, np.nan)

    def work(q):
        rf = Refined(gsz, inner=inner, division=div)
        try:
            sl = rf.hi.global_slice()
            rf.set_rhs(torch.from_numpy(np.ascontiguousarray(b[sl])).cuda())
            rf.set_field(p[sl])
            k = rf.solve()
            rf.get_field(X[sl])
            return k, list(rf.history)
        finally:
            rf.close()

    res = _ranks(4, ["f64", "f32"], work)
    assert all(r == res[0] for r in res)
    print("decomposed", res[0], "single", steps, hist)
    assert res[0][0] == steps and [h[2] for h in res[0][1]] == [h[2] for h in hist]
    assert _true_rel(b, p, X)[0] <= 1e-10


# ---- the stream hand-over
def test_stream_hand_over_of_both_entries():
    """on a non-default stream: the source of add_field is overwritten right after the call, the destination of get_residual is consumed right
    after it, work queued in front of both -- the results of the plain calls"""
    torch = _torch()
    gsz, scale = (64, 64, 64), 2.0 ** 9
    b, p, _, _ = _problem(gsz, "f64")
    e = (np.random.default_rng(3).random(gsz) - 0.5).astype(np.float32)
    x = RP.add(p, e, 0.25)
    want = RP.scaled(RP.residual(x, b, "f64"), scale, np.float32)
    cz = _handle("f64", list(gsz) + ["jacobi", 10, 0.8])
    try:
        cz.set_rhs(b)
        cz.set_field(p)
        s = torch.cuda.Stream()
        eh = torch.from_numpy(e).pin_memory()
        junk = torch.empty(256 * 1024 * 1024 // 8, dtype=torch.float64, device="cuda")
        et, rt = torch.empty(gsz, dtype=torch.float32, device="cuda"), torch.empty(gsz, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(8):
                junk.fill_(1.0)       # work in front of the final values, on the caller's stream
            et.fill_(123.0)
            et.copy_(eh, non_blocking=True)
            cz.add_field(et, 0.25)
            et.fill_(0.0)             # the caller may reuse its array at once
            junk.fill_(2.0)
            _, ss = cz.get_residual(out=rt, scale=scale)
            doubled = rt * 2.0        # consumed on the caller's stream, no synchronisation before it
            host = doubled.cpu()
        assert cz.get_field().tobytes() == x.tobytes()
        assert host.numpy().tobytes() == (want * 2.0).tobytes()
    finally:
        cz.close()
