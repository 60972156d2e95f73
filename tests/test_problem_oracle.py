"""A caller's own problem on the CPU (no GPU needed): the oracle wrapper of tests/problem_parity.py is harmless on the built-in problem, every
case tests/test_gpu_problem.py compares the GPU with converges on the oracle before its ItrMax (and, for the FP32 Krylov cases, fulfils the
premise of bit equality), and the libraries export the new entries."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cg_parity as CP  # noqa: E402
import problem_parity as PP  # noqa: E402
from cubez_amd import lib  # noqa: E402

NEW_SYMBOLS = ["cz_set_rhs", "cz_set_field", "cz_get_field", "cz_set_eps", "cz_set_itr_max"]
BUILTIN = [PP.case((24, 20, 28), s, cf, prec, n, pc=pc)
           for s, cf, n, pc in (("jacobi", 0.8, 200, None), ("sor2sma", 1.5, 100, None), ("psor", 1.5, 60, None), ("pcr_rb", 1.2, 40, None),
                                ("pcr", 1.2, 40, None), ("jacobi_maf", 0.8, 100, None), ("pbicgstab", 0.8, 30, "jacobi"), ("pcg", 0.8, 30, "jacobi"),
                                ("pcg", 1.0, 20, "mgrb"))
           for prec in ("f32", "f64")]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_libraries_export_the_new_entries(prec):
    """nm-level presence (the ABI test compares the header with cubez_amd.lib.ABI_SYMBOLS, which lists them too)"""
    out = subprocess.run(["nm", "-D", "--defined-only", lib.lib_path(prec)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in NEW_SYMBOLS if s not in exported]
    assert not [s for s in NEW_SYMBOLS if s not in lib.ABI_SYMBOLS]


@pytest.mark.parametrize("c", BUILTIN, ids=[c["id"] for c in BUILTIN])
def test_wrapper_is_harmless_on_the_builtin_problem(c):
    """bc_k as the identity after set-up: iterate, count and history of the unwrapped loop, bit for bit (no sweep writes a face)"""
    a, b = PP.run(c, builtin=True, wrapped=True), PP.run(c, builtin=True, wrapped=False)
    assert a.itr == b.itr and a.history == b.history and a.P.tobytes() == b.P.tobytes()
    assert a.itr > 0


def test_pad_and_unpad_are_inverse():
    a = np.arange(9 * 7 * 12, dtype=np.float32).reshape(9, 7, 12)
    P = PP.pad(a)
    assert P.shape == (11, 13, 16) and P[2 + 3, 2 + 5, 2 + 7] == a[5, 3, 7] and PP.unpad(P).tobytes() == a.tobytes()
    assert P[:2].max() == 0 and P[:, :2].max() == 0 and P[:, :, -2:].max() == 0


ALL = PP.CASES + [c for c, _ in PP.DECOMP]


@pytest.mark.parametrize("c", ALL, ids=[c["id"] for c in ALL])
def test_every_gpu_case_converges_on_the_oracle(c):
    r = PP.run(c)
    print(c["id"], "iterations", r.itr, "residual", r.res)
    assert PP.converged(c, r), (c["id"], r.itr, r.res)
    if PP.krylov(c) and c["prec"] == "f32":
        f = CP.flips(r, "f32")
        assert not f, f"{c['id']}: a dot within its summation bound of a float boundary {f[:4]}: choose another seed"
    if PP.krylov(c) and c["prec"] == "f64":
        o, E, Eh = PP.envelope_f64(c)
        assert float(E.max() / np.abs(o.P).max()) <= CP.ENVELOPE_MAX  # (or the bound would say nothing)


@pytest.mark.parametrize("c", PP.RESOLVE, ids=[c["id"] for c in PP.RESOLVE])
def test_resolve_cases_converge_twice(c):
    first, second = PP.resolve(c)
    assert PP.converged(c, first) and PP.converged(c, second)
    if c["solver"] == "jacobi":  # not the last sweep of a pass of two or of three: the driver must re-run the converged iteration alone
        assert second.itr % 2 == 1 and second.itr % 3 != 0, second.itr


def test_manufactured_solution_on_the_oracle():
    c = PP.case((64, 64, 64), "pcg", 1.0, "f64", 100, pc="mgrb", eps=1e-10)
    u, b, p = PP.manufactured(c["gsz"])
    r = PP.run(c, b=b, p=p)
    err = float(np.abs(PP.unpad(r.P) - u).max())
    print("manufactured: iterations", r.itr, "residual", r.res, "max error", err)
    assert PP.converged(c, r) and r.itr == 13
    assert err < 1e-9  # measured 7.73e-10: the residual test at 1e-10 stops there


def test_python_binding_refuses_before_the_library_is_called():
    """shape and dtype are checked against the brick in Python; cubez_amd imports without torch (this module never imported it)"""
    from cubez_amd import driver
    cz = driver.CZ.__new__(driver.CZ)
    cz.real, cz.device = np.float32, 0
    cz.local = lambda: dict(size=[9, 7, 12], head=[1, 1, 1])
    for bad in (np.zeros((9, 7, 12)), np.zeros((9, 7, 11), dtype=np.float32), [1.0, 2.0], np.zeros((9, 7, 12), dtype=np.float32)[::-1]):
        with pytest.raises(ValueError):
            cz._brick(bad, "set_field")
    ptr, strides, on_dev, stream, _ = cz._brick(np.zeros((12, 7, 9), dtype=np.float32).transpose(2, 1, 0), "set_field")
    assert strides == [1, 9, 63] and on_dev == 0 and stream is None
    from cubez_amd.decomp import brick_slice
    assert brick_slice([4, 5, 6], [1, 6, 13]) == (slice(0, 4), slice(5, 10), slice(12, 18))
