"""The zebra line smoother along Z (cz_set_mg_lines): its level-0 sweeps against a device-to-device copy of the bytes they
move, the V-cycle per label with lines on and off, and what it does to a solve on a stretched grid:
    python3 tools/lines_rate.py [n=512] [repeats=11] [solve_repeats=repeats]
Per precision, in one process, without torch (numpy fields, HIP events through ctypes).
Kernel: one V-cycle per call of cz_precondition, Dirichlet faces, pcg mgrb 1.0, stretch(30); median over the repeats after 3 warm-up calls of
the time the library's HIP events record under `rbsor` (level 0's eight colour sweeps), against hipMemcpyDtoDAsync of the bytes the line
kernel is modelled to move, in half arrays (the rows of one colour) per sweep:
    from the iterate   u(I+1), u(I-1), u(J+1), u(J-1), X(I), X(I-1), Y(J), Y(J-1), b, D, Z in (11); cp, dp out and in again (4); u in, x out (2) = 17
    first from zero    b, D, Z in (3); cp, dp out and in (4); x out (1)                                                                    =  8
    second from zero   the 11 in; cp, dp out and in (4); x out (1)                                                                         = 16
a cycle on Dirichlet faces runs one first, one second and six from the iterate: 126 half arrays = 63 array passes.
Cycle: every label of the cycle with lines off and on, on one handle.
Solves: the seeded problem to eps 1e-5 with anisoz(100), stretch(30) and random, pcg mgrb 1.0 under the coefficient hierarchy, lines
off / on / off / on on one handle: iterations, ms per iteration and ms to convergence (wall time of cz_solve), median (min, max) of the
repeats after one warm-up."""
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
LABELS = ("rbsor", "mg_rb", "mg_restrict", "mg_prolong", "mg_tail", "bc_mirror")


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


def stretch(R, ratio):
    """tests/lines_parity.stretch: cell heights ratio ** (t - 1) towards both Z walls, bx = by = h, bz = 2 / (h_k + h_{k+1})"""
    k = np.arange(n)
    h = float(ratio) ** (np.minimum(k, n - 1 - k) / (n / 2.0) - 1.0)
    bz = 2.0 / (h + np.roll(h, -1))
    return [np.ascontiguousarray(np.broadcast_to(v.astype(R), (n, n, n))) for v in (h, h, bz)]


def anisoz(R, ratio):
    return [np.full((n, n, n), v, dtype=R) for v in (1.0, 1.0, float(ratio))]


def random(R):
    rng = np.random.default_rng(3000)
    return [(0.5 + 1.5 * rng.random((n, n, n))).astype(R) for _ in range(3)]


def cycle_ms(cz, r):
    """time per V-cycle under every label: {label: ((median, min, max), launches)}"""
    for _ in range(3):
        cz.precondition(r)
    out = {lb: [] for lb in LABELS}
    cnt = {}
    for _ in range(reps):
        before = {lb: cz.timing_read(lb) for lb in LABELS}
        cz.precondition(r)
        for lb in LABELS:
            n1, t1 = cz.timing_read(lb)
            cnt[lb] = n1 - before[lb][0]
            out[lb].append(t1 - before[lb][1])
    return {lb: ((statistics.median(v), min(v), max(v)), cnt[lb]) for lb, v in out.items()}


for prec, R in (("f32", np.float32), ("f64", np.float64)):
    esz = np.dtype(R).itemsize
    cells = n ** 3
    rng = np.random.default_rng(1000)
    b = ((rng.random((n, n, n)) * 2.0 - 1.0) * 1e-2).astype(R)
    p = rng.random((n, n, n)).astype(R)
    rpad = np.zeros((n + 4, n + 4, n + 4), dtype=R)
    rpad[3:-3, 3:-3, 3:-3] = rng.standard_normal((n - 2, n - 2, n - 2)).astype(R)
    # -- the cycle per label, lines off and on; level 0's sweeps against the copy
    cz = CZ(prec, quiet=True)
    assert cz.setup([n, n, n, "pcg", 1, 1.0, "mgrb"]) == 1
    cz.set_face_coef(*stretch(R, 30))
    cz.set_coef_mg(True)
    cz.timing(True)
    for on in (False, True):
        cz.set_mg_lines(on)
        assert cz.info()["mg_lines"] == int(on)
        t = cycle_ms(cz, rpad)
        total = sum(v[0][0] for v in t.values())
        print(f"{prec} {n}^3  V-cycle, lines {int(on)}: " + ", ".join(f"{lb} {v[0][0]:.4f} ms ({v[1]} launches)" for lb, v in t.items()) + f"; sum {total:.4f} ms", flush=True)
        if on:
            passes = 63.0
            (med, lo, hi), cnt = t["rbsor"]
            assert cnt == 8, cnt
            cp = copy_ms(int(passes * cells * esz / 2))
            print(f"{prec} {n}^3  rbsor (lines): {cnt} colour sweeps per cycle, median {med:.4f} ms (min {lo:.4f}, max {hi:.4f}), {med / cnt:.4f} ms per sweep;  "
                  f"{passes:.1f} array passes, {passes * cells * esz / med / 1e6:.0f} GB/s;  the copy of its bytes: median {cp[0]:.4f} ms (min {cp[1]:.4f}, "
                  f"max {cp[2]:.4f})  = {med / cp[0]:.2f} x the copy", flush=True)
    cz.timing(False)
    cz.close()
    # -- the solves: lines off / on / off / on
    cz = CZ(prec, quiet=True)
    assert cz.setup([n, n, n, "pcg", 2000, 1.0, "mgrb"]) == 1
    cz.set_eps(1e-5)
    cz.set_rhs(b)
    for name, beta in (("anisoz100", anisoz(R, 100)), ("stretch30", stretch(R, 30)), ("random", random(R))):
        cz.set_face_coef(*beta)
        cz.set_coef_mg(True)
        for on in (False, True, False, True):
            cz.set_mg_lines(on)
            assert cz.info()["mg_lines"] == int(on) and cz.info()["coef_mg"] == 1
            per, tot, its = [], [], 0
            for rr in range(1 + sreps):
                cz.set_field(p)
                its = cz.solve()
                if rr >= 1:
                    tot.append(cz.solve_seconds * 1e3)
                    per.append(cz.solve_seconds * 1e3 / max(its, 1))
            print(f"{prec} {n}^3  pcg mgrb 1.0 {name:10s} lines {int(on)}: {its} iterations to eps 1e-5, {statistics.median(per):.3f} ms per iteration "
                  f"(min {min(per):.3f}, max {max(per):.3f}), {statistics.median(tot):.1f} ms to convergence (min {min(tot):.1f}, max {max(tot):.1f})", flush=True)
        del beta
    cz.close()
    del b, p, rpad
