"""jac4_k (four Jacobi sweeps per pass) against jac3_k and the two-sweep pass (jacobi2p_k): ms per sweep, MLUPS, by window length and chunk.
    python3 tools/jac4_rate.py prec n [kwin,tj ...]
The pair line is the untouched yardstick of a call: its scatter between calls is the scatter a jac4 / jac3 ratio has to beat."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from cubez_amd import CzHip

prec, n = sys.argv[1], int(sys.argv[2])
forms = [tuple(int(v) for v in a.split(",")) for a in sys.argv[3:]] or [(0, 0)]
h = CzHip(prec)
R = h.real
sz, idx = [n, n, n], [2, n - 1, 2, n - 1, 2, n - 1]
rng = np.random.default_rng(1)
shape = (n + 4, n + 4, n + 4)
cf = np.array([1, 1, 1, 1, 1, 1, 6], dtype=R)
p = rng.uniform(-1, 1, shape).astype(R)
du, db, dw = h.alloc(sz, p), h.alloc(sz, p * 0), h.alloc(sz, p)
(_, szp), (_, idxp), (_, cfp) = h._i(sz), h._i(idx), h._r(cf)
dres = h.lib.czhip_alloc_s3d((C.c_int * 3)(4, 4, 4))
f2 = h.lib.czhip_jacobi2_async
f2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, h.creal, C.c_void_p, C.c_double, C.c_double,
               C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
deep = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, h.creal, C.c_void_p, C.c_double, C.c_double, C.c_int,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
f3, f4 = h.lib.czhip_jacobi3_async, h.lib.czhip_jacobi4_async
f3.argtypes = f4.argtypes = deep
pts = (n - 2) ** 3


def run(fn, reps):
    a, b = du, dw
    for _ in range(5):
        fn(a, b)
        a, b = b, a
    h.sync()
    best = 1e9
    for rep in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn(a, b)
            a, b = b, a
        h.sync()
        best = min(best, (time.perf_counter() - t0) / reps)
    return best


def deep_call(f, a, b, probe):
    return f(a.ptr, b.ptr, db.ptr, szp, idxp, 2, cfp, 0.8, dres, 0.0, 0.0, 0, None, None, None, None, probe)


reps = max(6, int(60 * (512 / n) ** 3))
t2 = run(lambda a, b: f2(a.ptr, b.ptr, db.ptr, szp, idxp, None, 2, cfp, 0.8, dres, 0.0, 0.0, 0, None, None, None, None), reps)
print(f"{prec} {n}^3  two sweeps per pass (jacobi2p_k): {t2 * 1e3:.4f} ms per pass = {t2 * 5e2:.4f} ms per sweep  {2 * pts / t2 / 1e6:9.0f} MLUPS", flush=True)
h.lib.czhip_set_jac3(2, 0, 0)
t3 = None
if deep_call(f3, du, dw, 1):
    t3 = run(lambda a, b: deep_call(f3, a, b, 0), reps)
    print(f"   jac3 (the launcher's rule):  {t3 * 1e3:.4f} ms per pass = {t3 / 3 * 1e3:.4f} ms per sweep  {3 * pts / t3 / 1e6:9.0f} MLUPS  ({(t2 / 2) / (t3 / 3):.3f} x the pair)", flush=True)
for kw, tj in forms:
    h.lib.czhip_set_jac4(2, kw, tj)
    if not deep_call(f4, du, dw, 1):
        print(f"   jac4 window {kw} chunk {tj}: refused")
        continue
    t4 = run(lambda a, b: deep_call(f4, a, b, 0), reps)
    vs3 = f"  {(t3 / 3) / (t4 / 4):.3f} x jac3" if t3 else ""
    print(f"   jac4 window {kw:3d} chunk {tj:3d}: {t4 * 1e3:.4f} ms per pass = {t4 / 4 * 1e3:.4f} ms per sweep  {4 * pts / t4 / 1e6:9.0f} MLUPS  ({(t2 / 2) / (t4 / 4):.3f} x the pair{vs3})", flush=True)
h.lib.czhip_set_jac4(1, 0, 0)
h.lib.czhip_set_jac3(1, 0, 0)
