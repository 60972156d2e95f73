"""The coefficient hierarchy (cz_set_coef_mg): its level-0 kernels against a device-to-device copy of the bytes they move,
and what it does to a solve with a sharp jump:
    python3 tools/coefmg_rate.py [n=512] [repeats=11] [solve_repeats=repeats]
Per precision, in one process, without torch (numpy fields, HIP events through ctypes).
Kernels: one V-cycle per call of cz_precondition, Dirichlet faces; median over the repeats after 3 warm-up calls of the time the library's
HIP events record under a label per cycle, against hipMemcpyDtoDAsync of the bytes of the level-0 launches under that label:
    jacobi       (pcg mg)    1 sweep from zero (b, D in, w out: 3 array passes) + 3 sweeps (u, b, X, Y, Z, D in, w out: 7)      = 24 passes
    rbsor        (pcg mgrb)  8 colour sweeps in place: the first from zero (x, b, D in, x out: 4), seven with x, b, X, Y, Z, D in, x out = 53 passes
    mg_restrict  (either)    residual + restriction, x, b, X, Y, Z, D in, an eighth of an array out; the label also holds the same launch
                             of the levels above the tail (an eighth, a 64th ... of the bytes: counted)
Solves: the seeded problem to eps 1e-5 with bubble(1000) and smooth(4), pcg mgrb 1.2 and pcg mg 0.8, the flag off / on / off / on on one
handle: iterations, ms per iteration and ms to convergence (wall time of cz_solve), median (min, max) of the repeats after one warm-up."""
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cubez_amd import CZ  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 11
sreps = int(sys.argv[3]) if len(sys.argv) > 3 else reps
hip = C.CDLL("libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipFree.argtypes = [C.c_void_p]
hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]


def check(e):
    assert e == 0, f"HIP error {e}"


def copy_ms(nbytes):
    """hipMemcpyDtoDAsync of nbytes (read + write: 2 nbytes moved), events on the null stream: median, min, max"""
    src, dst, a, b = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    check(hip.hipMalloc(C.byref(src), nbytes)), check(hip.hipMalloc(C.byref(dst), nbytes))
    check(hip.hipMemset(src, 1, nbytes))
    check(hip.hipEventCreate(C.byref(a))), check(hip.hipEventCreate(C.byref(b)))
    out = []
    for r in range(3 + reps):
        check(hip.hipEventRecord(a, None))
        check(hip.hipMemcpyDtoDAsync(dst, src, nbytes, None))
        check(hip.hipEventRecord(b, None))
        check(hip.hipEventSynchronize(b))
        ms = C.c_float()
        check(hip.hipEventElapsedTime(C.byref(ms), a, b))
        if r >= 3:
            out.append(ms.value)
    hip.hipFree(src), hip.hipFree(dst)
    return statistics.median(out), min(out), max(out)


def face_points(ax):
    pts = []
    for d in range(3):
        c = (np.arange(n) + (0.5 if d == ax else 0.0)) / (n - 1.0)
        pts.append(c.reshape([-1 if q == d else 1 for q in range(3)]))
    return pts


def bubble(R, ratio):
    """tests/coef_parity.bubble: `ratio` on the faces whose centre lies in a ball of radius 0.25 about the middle of the box, 1 elsewhere"""
    out = []
    for ax in range(3):
        x, y, z = face_points(ax)
        inside = (x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2 < 0.25 ** 2
        out.append(np.ascontiguousarray(np.broadcast_to(np.where(inside, float(ratio), 1.0), (n, n, n))).astype(R))
    return out


def smooth(R, ratio):
    """tests/coef_parity.smooth: ratio ** (a product of three sines scaled to [0, 1])"""
    out = []
    for ax in range(3):
        x, y, z = face_points(ax)
        f = 0.5 * (1.0 + np.sin(2.0 * np.pi * x) * np.sin(2.0 * np.pi * y) * np.sin(2.0 * np.pi * z))
        out.append(np.ascontiguousarray(np.broadcast_to(float(ratio) ** f, (n, n, n))).astype(R))
    return out


def cycle_ms(cz, r, label, launches_min):
    """time under `label` per V-cycle: median, min, max; the launches per cycle"""
    for _ in range(3):
        cz.precondition(r)
    out, cnt = [], 0
    for _ in range(reps):
        n0, t0 = cz.timing_read(label)
        cz.precondition(r)
        n1, t1 = cz.timing_read(label)
        cnt = n1 - n0
        assert cnt >= launches_min, (label, cnt)
        out.append(t1 - t0)
    return (statistics.median(out), min(out), max(out)), cnt


for prec, R in (("f32", np.float32), ("f64", np.float64)):
    esz = np.dtype(R).itemsize
    cells = n ** 3
    rng = np.random.default_rng(1000)
    b = ((rng.random((n, n, n)) * 2.0 - 1.0) * 1e-2).astype(R)
    p = rng.random((n, n, n)).astype(R)
    fields = {"bubble1000": bubble(R, 1000), "smooth4": smooth(R, 4)}
    rpad = np.zeros((n + 4, n + 4, n + 4), dtype=R)
    rpad[3:-3, 3:-3, 3:-3] = rng.standard_normal((n - 2, n - 2, n - 2)).astype(R)
    # -- the level-0 kernels
    for pc, coef, label, passes, launches in (("mg", 0.8, "jacobi", 24.0, 4), ("mgrb", 1.2, "rbsor", 53.0, 8), ("mg", 0.8, "mg_restrict", 6.125 * 8.0 / 7.0, 1)):
        cz = CZ(prec, quiet=True)
        assert cz.setup([n, n, n, "pcg", 1, coef, pc]) == 1
        cz.set_face_coef(*fields["bubble1000"])
        cz.set_coef_mg(True)
        assert cz.info()["coef_mg"] == 1
        cz.timing(True)
        t, cnt = cycle_ms(cz, rpad, label, launches)
        cz.timing(False)
        cz.close()
        nbytes = int(passes * cells * esz / 2)
        cp = copy_ms(nbytes)
        print(f"{prec} {n}^3  {label:11s} ({pc}): {cnt} launches per cycle, median {t[0]:.4f} ms (min {t[1]:.4f}, max {t[2]:.4f})  {passes:.2f} array passes, "
              f"{passes * cells * esz / t[0] / 1e6:.0f} GB/s;  the copy of its bytes: median {cp[0]:.4f} ms (min {cp[1]:.4f}, max {cp[2]:.4f})  "
              f"= {t[0] / cp[0]:.2f} x the copy", flush=True)
    # -- the solves: the flag off / on / off / on
    for pc, coef in (("mgrb", 1.2), ("mg", 0.8)):
        cz = CZ(prec, quiet=True)
        assert cz.setup([n, n, n, "pcg", 1000, coef, pc]) == 1
        cz.set_eps(1e-5)
        cz.set_rhs(b)
        for name, beta in fields.items():
            cz.set_face_coef(*beta)
            for on in (False, True, False, True):
                cz.set_coef_mg(on)
                per, tot, its = [], [], 0
                for rr in range(1 + sreps):
                    cz.set_field(p)
                    its = cz.solve()
                    if rr >= 1:
                        tot.append(cz.solve_seconds * 1e3)
                        per.append(cz.solve_seconds * 1e3 / max(its, 1))
                print(f"{prec} {n}^3  pcg {pc} {coef} {name:10s} coef_mg {int(on)}: {its} iterations to eps 1e-5, {statistics.median(per):.3f} ms per iteration "
                      f"(min {min(per):.3f}, max {max(per):.3f}), {statistics.median(tot):.1f} ms to convergence (min {min(tot):.1f}, max {max(tot):.1f})", flush=True)
        cz.close()
    del b, p, fields, rpad
