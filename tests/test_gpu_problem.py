"""A caller's own problem through cz_set_rhs / cz_set_field / cz_get_field / cz_set_eps / cz_set_itr_max on the GPU (-m gpu): the import and
export kernels byte for byte, every solver family against the oracle on a caller's problem (tests/problem_parity.py), the faces of the
right-hand side, decomposed runs, repeated solves, the stream hand-over and a manufactured solution.

Bars are those of the existing tests of each family: stationary and line solvers bit for bit against the wide oracle, Krylov FP32 bit for bit
and FP64 within 2 E + 8 ulp of the exact-dot oracle (E: the envelope of the runs with every dot at either edge of its summation bound).
"""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import problem_parity as PP  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
G = PP.G


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    return torch


def _handle(prec, a):
    from cubez_amd import CZ
    cz = CZ(prec, quiet=True)
    assert cz.setup(a) == 1
    return cz


def _real(prec):
    return np.float32 if prec == "f32" else np.float64


# ---- the layouts a caller's array [i, j, k] comes in: name -> (array to fill, view indexed [i, j, k]); xp = numpy or torch
def _layouts(xp, shape, dtype, **kw):
    ni, nj, nk = shape
    out = {}
    a = xp.zeros((ni, nj, nk), dtype=dtype, **kw)
    out["c_order"] = (a, a)                                     # k is the unit stride: rows
    a = xp.zeros((nk, nj, ni), dtype=dtype, **kw)
    out["fortran"] = (a, a.permute(2, 1, 0) if hasattr(a, "permute") else a.transpose(2, 1, 0))   # i is the unit stride: transpose
    a = xp.zeros((nj, nk, ni), dtype=dtype, **kw)
    out["perm_jki"] = (a, a.permute(2, 0, 1) if hasattr(a, "permute") else a.transpose(2, 0, 1))  # i unit, k before j
    a = xp.zeros((ni, nk, nj), dtype=dtype, **kw)
    out["perm_ikj"] = (a, a.permute(0, 2, 1) if hasattr(a, "permute") else a.transpose(0, 2, 1))  # j is the unit stride: transpose
    a = xp.zeros((ni + 3, nj + 2, nk + 5), dtype=dtype, **kw)
    out["slice"] = (a, a[2:2 + ni, 1:1 + nj, 3:3 + nk])         # rows that start anywhere
    a = xp.zeros((ni, nj, 2 * nk), dtype=dtype, **kw)
    out["every_other"] = (a, a[:, :, ::2])                      # no unit stride: generic
    return out


FORM = {"c_order": 1, "fortran": 2, "perm_jki": 2, "perm_ikj": 2, "slice": 1, "every_other": 3}


@pytest.mark.parametrize("force", [0, 3], ids=["form_by_strides", "generic_forced"])
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", PP.BOXES + [(5, 70, 130)], ids=lambda g: "x".join(map(str, g)))
def test_import_and_export_move_exactly_the_brick(gsz, prec, where, force, monkeypatch):
    """set_field then cz_field equals the numpy-padded array byte for byte, guide cells as set-up left them; get_field into a sentinel-filled
    destination writes exactly the brick; every layout, both kernel forms of it (CZ_FIELD_FORM=3: the generic one)"""
    R = _real(prec)
    if force:
        monkeypatch.setenv("CZ_FIELD_FORM", str(force))
    if where == "device":
        torch = _torch()
        xp, kw, tdt = torch, dict(device="cuda"), torch.float32 if prec == "f32" else torch.float64
    else:
        xp, kw, tdt = np, {}, R
    cz = _handle(prec, list(gsz) + ["jacobi", 10, 0.8])
    try:
        before = cz.field()
        rng = np.random.default_rng(7)
        for name, (base, view) in _layouts(xp, gsz, tdt, **kw).items():
            vals = rng.random(gsz).astype(R)
            if where == "device":
                view.copy_(torch.from_numpy(vals).cuda())
            else:
                view[...] = vals
            cz.set_field(view)
            assert cz.info()["field_form"] == (3 if force else FORM[name]), (name, cz.info()["field_form"])
            assert cz.field().tobytes() == PP.pad(vals, into=before).tobytes(), f"{name}: the padded array differs"
            # export into sentinels
            if where == "device":
                base.fill_(-77.0)
            else:
                base[...] = -77.0
            cz.get_field(view)
            got = base.cpu().numpy() if where == "device" else base
            want = np.full(got.shape, -77.0, dtype=R)
            (want.transpose(2, 1, 0) if name == "fortran" else want.transpose(2, 0, 1) if name == "perm_jki" else want.transpose(0, 2, 1) if name == "perm_ikj"
             else want[2:2 + gsz[0], 1:1 + gsz[1], 3:3 + gsz[2]] if name == "slice" else want[:, :, ::2] if name == "every_other" else want)[...] = vals
            assert got.tobytes() == want.tobytes(), f"{name}: the export wrote something else than the brick"
        # the right-hand side goes the same way and leaves P alone
        b = rng.random(gsz).astype(R)
        cz.set_rhs(b if where == "host" else torch.from_numpy(b).cuda())
        assert cz.get_field().tobytes() == vals.tobytes()
    finally:
        cz.close()


def test_refusals_leave_the_handle_usable():
    from cubez_amd import CZ
    cz = CZ("f32", quiet=True)
    a = np.zeros((9, 7, 12), dtype=np.float32)
    st = (C.c_longlong * 3)(84, 12, 1)
    assert cz.lib.cz_set_rhs(cz.h, a.ctypes.data, st, 0, None) == 0      # before cz_setup
    assert cz.lib.cz_set_eps(cz.h, 1e-6) == 0
    assert cz.setup([9, 7, 12, "jacobi", 50, 0.8]) == 1
    assert cz.lib.cz_set_rhs(cz.h, None, st, 0, None) == 0                # NULL
    assert cz.lib.cz_set_field(cz.h, a.ctypes.data, (C.c_longlong * 3)(84, 0, 1), 0, None) == 0  # a stride < 1
    assert cz.lib.cz_get_field(cz.h, a.ctypes.data, (C.c_longlong * 3)(1, 1, 1), 0, None) == 0    # cells of the destination alias
    assert cz.lib.cz_get_field(cz.h, a.ctypes.data, st, 1, None) == 0     # host memory offered as device memory
    assert cz.lib.cz_set_eps(cz.h, 0.0) == 0 and cz.lib.cz_set_eps(cz.h, -1.0) == 0
    assert cz.lib.cz_set_itr_max(cz.h, 0) == 0
    with pytest.raises(ValueError):
        cz.set_field(np.zeros((9, 7, 12), dtype=np.float64))
    with pytest.raises(ValueError):
        cz.set_field(np.zeros((9, 7, 13), dtype=np.float32))
    o = O.run((9, 7, 12), "jacobi", 50, 0.8, kind="oracle", prec="f32", wide=True)
    assert cz.solve() == o.itr and cz.field().tobytes() == o.P.tobytes()   # the built-in problem, untouched by the refusals
    cz.close()


# ---- solver parity on a caller's problem
def _gpu(c, b, p, eps=None, itr_max=None, fmt="host"):
    cz = _handle(c["prec"], PP.args(c))
    try:
        if fmt == "device":
            torch = _torch()
            b, p = torch.from_numpy(b).cuda(), torch.from_numpy(np.asfortranarray(p)).cuda()  # one row form, one transpose form
        cz.set_rhs(b)
        cz.set_field(p)
        if eps is not None:
            cz.set_eps(eps)
        if itr_max is not None:
            cz.set_itr_max(itr_max)
        itr = cz.solve()
        return dict(itr=itr, hist=list(cz.history()), P=cz.field(), X=cz.get_field(), info=cz.info())
    finally:
        cz.close()


def _compare(c, g, **kw):
    if not PP.krylov(c) or c["prec"] == "f32":
        o = PP.run(c, **kw)
        oh = [r for _, r in o.history]
        assert g["itr"] == o.itr, (c["id"], g["itr"], o.itr)
        assert g["P"].tobytes() == o.P.tobytes(), f"{c['id']}: field differs from the oracle"
        if PP.krylov(c):
            assert g["hist"] == oh, c["id"]
        else:  # (the bar of tests/test_gpu_solvers.py: the same double-accumulated terms in another order)
            assert len(g["hist"]) == len(oh) and np.allclose(g["hist"], oh, rtol=1e-11, atol=0), c["id"]
    else:
        o, E, Eh = PP.envelope_f64(c, **kw)
        assert g["itr"] == o.itr, (c["id"], g["itr"], o.itr)
        ok, worst = PP.f64_close(g["P"], o.P, E)
        assert ok, f"{c['id']}: field beyond the derived bound (worst |d| / bound = {worst:.3g})"
        h0 = [r for _, r in o.history]
        assert len(g["hist"]) == len(h0)
        ok, worst = PP.f64_close(g["hist"], h0, Eh)
        assert ok, f"{c['id']}: history beyond the derived bound (worst |d| / bound = {worst:.3g})"
    assert g["X"].tobytes() == PP.unpad(g["P"]).tobytes()
    return o


@pytest.mark.parametrize("c", PP.CASES, ids=[c["id"] for c in PP.CASES])
def test_solver_parity_on_a_callers_problem(c):
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    o = _compare(c, _gpu(c, b, p, fmt="device" if c["gsz"] == (33, 47, 61) else "host"))
    assert PP.converged(c, o)


@pytest.mark.parametrize("c", [PP.CASES[0], PP.CASES[2], PP.CASES[10]], ids=lambda c: c["id"])
def test_set_eps_and_set_itr_max_follow_the_oracle(c):
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    _compare(c, _gpu(c, b, p, eps=1e-3), eps=1e-3)
    g = _gpu(c, b, p, eps=1e-12, itr_max=7)
    o = _compare(c, g, eps=1e-12, itr_max=7)
    assert len(g["hist"]) == len(o.history) == (6 if c["solver"] == "pbicgstab" else 7)


# ---- values of the right-hand side on physical faces
def _faces_changed(b):
    b2 = b.copy()
    for ax in range(3):
        for side in (0, -1):
            sl = [slice(None)] * 3
            sl[ax] = side
            b2[tuple(sl)] = 1e3
    return b2


@pytest.mark.parametrize("c", [PP.CASES[0], PP.CASES[6], PP.CASES[8], PP.CASES[13]], ids=lambda c: c["id"])
def test_rhs_on_physical_faces_does_not_matter(c):
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    g1, g2 = _gpu(c, b, p), _gpu(c, _faces_changed(b), p)
    assert g1["itr"] == g2["itr"] and g1["hist"] == g2["hist"] and g1["P"].tobytes() == g2["P"].tobytes()


# ---- decomposed runs on the LOCAL transport: every rank imports its slice of one global array
def _decomposed(c, div, b, p):
    from cubez_amd import CZ, load
    lib = load(c["prec"])
    lib.cz_comm_local_world.restype = C.c_void_p
    lib.cz_comm_bootstrap_local.argtypes = [C.c_void_p, C.c_int]
    lib.cz_comm_local_world_free.argtypes = [C.c_void_p]
    n = div[0] * div[1] * div[2]
    world = lib.cz_comm_local_world(n)
    results, errors = [None] * n, []
    X = np.full(c["gsz"], np.nan, dtype=b.dtype)

    def work(r):
        try:
            lib.cz_comm_bootstrap_local(world, r)
            cz = CZ(c["prec"], quiet=True)
            assert cz.setup(PP.args(c, div)) == 1
            sl = cz.global_slice()
            cz.set_rhs(b[sl])  # (non-contiguous slices of the global arrays)
            cz.set_field(p[sl])
            itr = cz.solve()
            cz.get_field(X[sl])
            results[r] = (itr, list(cz.history()), cz.info())
            cz.close()
        except BaseException as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(n)]
    [t.start() for t in th]
    [t.join(timeout=90) for t in th]
    if any(t.is_alive() for t in th):  # a rank stuck in a collective cannot be unblocked (as tests/test_gpu_decomp.py)
        sys.stderr.write(f"DEADLOCK: decomposed {c['id']} {div} did not finish in 90 s\n")
        sys.stderr.flush()
        os._exit(3)
    assert not errors, errors
    lib.cz_comm_local_world_free(world)
    assert all(r[0] == results[0][0] and r[1] == results[0][1] for r in results)
    return results[0][0], results[0][1], X


DECOMP = PP.DECOMP


@pytest.mark.parametrize("c,div", DECOMP, ids=[f"{c['id']}_{'x'.join(map(str, d))}" for c, d in DECOMP])
def test_decomposed_import_equals_single_domain(c, div):
    """the gathered result under the rule tests/test_gpu_decomp.py and tests/test_gpu_pcg.py have for the solver: Jacobi and red-black SOR equal
    the single-domain run bit for bit; PCG lies within the exact-dot oracle's bound (FP32: bit for bit), its all-reduce being one more
    summation order"""
    b, p = PP.problem(c["gsz"], c["prec"], c["seed"])
    itr, hist, X = _decomposed(c, div, b, p)
    if not PP.krylov(c):
        g = _gpu(c, b, p)
        assert itr == g["itr"] and X.tobytes() == g["X"].tobytes()
        assert len(hist) == len(g["hist"]) and np.allclose(hist, g["hist"], rtol=1e-12, atol=0)  # (the rule of tests/test_gpu_decomp.py)
    else:
        P = PP.pad(X)
        _compare(c, dict(itr=itr, hist=hist, P=P, X=X))
    # the faces of b do not matter under a cut either
    itr2, hist2, X2 = _decomposed(c, div, _faces_changed(b), p)
    assert itr2 == itr and hist2 == hist and X2.tobytes() == X.tobytes()


def test_mgrb_stays_refused_on_more_than_one_rank(tmp_path):
    """two ranks as threads of a child process (as tests/test_gpu_mgrb.py): the set-up is refused, so there is nothing to import into"""
    import subprocess
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = textwrap.dedent(f"""
        import ctypes as C, sys, threading
        sys.path.insert(0, {root!r})
        from cubez_amd import CZ, load
        lib = load("f64")
        lib.cz_comm_local_world.restype = C.c_void_p
        lib.cz_comm_bootstrap_local.argtypes = [C.c_void_p, C.c_int]
        world = lib.cz_comm_local_world(2)
        def work(q):
            lib.cz_comm_bootstrap_local(world, q)
            cz = CZ("f64", quiet=True)
            cz.setup([32, 36, 40, "pcg", 10, 1.0, "mgrb", 2, 1, 1])
            print("SET UP", flush=True)
        th = [threading.Thread(target=work, args=(q,)) for q in range(2)]
        [t.start() for t in th]
        [t.join(timeout=60) for t in th]
        print("NOT REFUSED", flush=True)
        """)
    r = subprocess.run([sys.executable, "-c", child], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-600:])
    assert "pcg with mgrb runs on a single domain only (2 ranks)" in r.stdout, r.stdout
    assert "SET UP" not in r.stdout and "NOT REFUSED" not in r.stdout, r.stdout


# ---- solve, change the right-hand side, solve again from the last iterate
RESOLVE = PP.RESOLVE


@pytest.mark.parametrize("c", RESOLVE, ids=lambda c: c["id"])
def test_second_solve_equals_a_fresh_handle(c):
    b1, p = PP.problem(c["gsz"], c["prec"], 0)
    b2, _ = PP.problem(c["gsz"], c["prec"], PP.RESOLVE_SEED)
    cz = _handle(c["prec"], PP.args(c))
    try:
        cz.set_rhs(b1)
        cz.set_field(p)
        assert cz.solve() > 0
        x1 = cz.get_field()
        cz.set_rhs(b2)
        itr = cz.solve()
        second = (itr, list(cz.history()), cz.field().tobytes(), cz.info())
    finally:
        cz.close()
    g = _gpu(c, b2, x1)
    assert (g["itr"], g["hist"], g["P"].tobytes()) == second[:3]
    assert 0 < itr <= c["itr_max"]
    if c["solver"] == "jacobi":
        # (a converged iteration that is not the last of its fused pass is re-run alone from the pass's input: the second solve took that path
        # exactly as the fresh handle did)
        assert second[3]["exact_reruns"] == g["info"]["exact_reruns"]
        print("jacobi re-solve: iterations", itr, "exact_reruns", second[3]["exact_reruns"])
        assert second[3]["exact_reruns"] == 1, (itr, second[3])


# ---- the stream hand-over
def test_stream_hand_over_without_device_synchronisation():
    """a tensor produced on a non-default stream immediately before set_rhs (a large fill, then the final values) is imported complete; the
    exported tensor is consumed on the caller's stream without any synchronisation in between"""
    torch = _torch()
    c = PP.case((64, 64, 64), "pcg", 1.0, "f64", 100, pc="mgrb")
    b, p = PP.problem(c["gsz"], c["prec"], 3)
    want = _gpu(c, b, p)
    cz = _handle(c["prec"], PP.args(c))
    try:
        s = torch.cuda.Stream()
        bh, ph = torch.from_numpy(b).pin_memory(), torch.from_numpy(p).pin_memory()
        junk = torch.empty(256 * 1024 * 1024 // 8, dtype=torch.float64, device="cuda")
        bt, pt, out = (torch.empty(c["gsz"], dtype=torch.float64, device="cuda") for _ in range(3))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(8):
                junk.fill_(1.0)          # work in front of the final values, on the caller's stream
            bt.fill_(123.0)
            pt.fill_(-5.0)
            bt.copy_(bh, non_blocking=True)
            pt.copy_(ph, non_blocking=True)
            cz.set_rhs(bt)
            cz.set_field(pt)
            bt.fill_(0.0)                # the caller may reuse its arrays at once
            itr = cz.solve()
            cz.get_field(out)
            doubled = out * 2.0          # consumed on the caller's stream, no synchronisation before it
            host = doubled.cpu()
        assert itr == want["itr"]
        assert host.numpy().tobytes() == (want["X"] * 2.0).tobytes()
    finally:
        cz.close()


# ---- a manufactured solution, as a user would check the library
def test_manufactured_solution_pcg_mgrb_64_f64():
    """b = A u for a smooth u (the oracle's blas_calc_ax), u's faces as Dirichlet values, zero guess inside, eps 1e-10: the GPU's max error
    against u is at most the wrapped oracle's plus the FP64 bar of the parity cases (2 E + 8 ulp, E from the perturbed oracle runs).
    Measured on the CPU: the oracle converges in 13 iterations (residual 5.11e-11) with max |p - u| = 7.73e-10
    (tests/test_problem_oracle.py asserts both)."""
    c = PP.case((64, 64, 64), "pcg", 1.0, "f64", 100, pc="mgrb", eps=1e-10)
    u, b, p = PP.manufactured(c["gsz"])
    g = _gpu(c, b, p, eps=c["eps"])
    r = {q: PP.run(c, b=b, p=p, perturb=q) for q in (-1, 0, 1)}
    assert r[-1].itr == r[0].itr == r[1].itr == g["itr"] < c["itr_max"]
    err = {q: float(np.abs(PP.unpad(r[q].P) - u).max()) for q in r}
    E = max(abs(err[1] - err[0]), abs(err[-1] - err[0]))
    gerr = float(np.abs(g["X"] - u).max())
    print("manufactured: oracle error", err[0], "GPU error", gerr, "envelope", E)
    assert gerr <= err[0] + 2.0 * E + 8.0 * np.spacing(np.abs(u).max())
