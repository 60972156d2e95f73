"""Import / export of a caller's field (cz_set_field, cz_get_field) against a device-to-device copy of one padded array:
    python3 tools/field_io_rate.py [n=512] [repeats=11]
Per precision and layout: median kernel time over the repeats (HIP events around the launch, label field_io) after 3 warm-up calls, the
bytes moved (brick read + brick written) and the rate; the yardstick is hipMemcpyDtoDAsync of (n+4)^3 elements timed in the same process
with events on the same stream.  Last: one FP64 pcg mgrb solve with and without import + export (wall clock, device tensors)."""
import ctypes as C
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cubez_amd import CZ  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 11
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]


def label_ms(cz, fn):
    """median kernel time of fn()'s field_io launch over the repeats"""
    for _ in range(3):
        fn()
    out = []
    for _ in range(reps):
        n0, t0 = cz.timing_read("field_io")
        fn()
        cz.lib.czhip_sync()
        n1, t1 = cz.timing_read("field_io")
        assert n1 - n0 == 1
        out.append(t1 - t0)
    return statistics.median(out), min(out), max(out)


for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
    esz = 4 if prec == "f32" else 8
    cz = CZ(prec, quiet=True)
    assert cz.setup([n, n, n, "jacobi", 10, 0.8]) == 1
    cz.timing(True)
    s = torch.cuda.Stream()
    pad_elems = (n + 4) ** 3
    src, dst = torch.ones(pad_elems, dtype=dt, device="cuda"), torch.empty(pad_elems, dtype=dt, device="cuda")
    torch.cuda.synchronize()
    times = []
    for r in range(3 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        assert hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), pad_elems * esz, s.cuda_stream) == 0
        b.record(s)
        s.synchronize()
        if r >= 3:
            times.append(a.elapsed_time(b))
    cp = statistics.median(times)
    print(f"{prec} {n}^3  hipMemcpyDtoDAsync of one padded array: median {cp:.4f} ms (min {min(times):.4f}, max {max(times):.4f})  "
          f"{2 * pad_elems * esz / cp / 1e6:.0f} GB/s  = {cp / pad_elems * 1e6:.4f} ns per element", flush=True)
    del src, dst
    c_order = torch.rand((n, n, n), dtype=dt, device="cuda")
    f_order = torch.rand((n, n, n), dtype=dt, device="cuda").permute(2, 1, 0)
    every = torch.rand((n, n, 2 * n), dtype=dt, device="cuda")[:, :, ::2] if prec == "f32" else None
    torch.cuda.synchronize()
    for name, t in (("C order (rows)", c_order), ("Fortran order (transpose)", f_order), ("k stride 2 (generic)", every)):
        if t is None:
            continue
        with torch.cuda.stream(s):
            for what, fn in (("import", lambda: cz.set_field(t)), ("export", lambda: cz.get_field(t))):
                med, lo, hi = label_ms(cz, fn)
                per = med / n ** 3 * 1e6
                print(f"{prec} {n}^3  {what} {name:26s}: median {med:.4f} ms (min {lo:.4f}, max {hi:.4f})  {2 * n ** 3 * esz / med / 1e6:.0f} GB/s  "
                      f"{per:.4f} ns per cell = {per / (cp / pad_elems * 1e6):.2f} x the copy per element  (form {cz.info()['field_form']})", flush=True)
    cz.close()
    del c_order, f_order, every

# the share in a solve
prec, dt = "f64", torch.float64
cz = CZ(prec, quiet=True)
assert cz.setup([n, n, n, "pcg", 100, 1.0, "mgrb"]) == 1
b = (torch.rand((n, n, n), dtype=dt, device="cuda") * 2 - 1) * 1e-2
p = torch.rand((n, n, n), dtype=dt, device="cuda")
out = torch.empty_like(p)
for rep in range(3):
    cz.set_rhs(b)
    cz.set_field(p)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    itr = cz.solve()
    t_solve = time.perf_counter() - t0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cz.set_rhs(b)
    cz.set_field(p)
    itr2 = cz.solve()
    cz.get_field(out)
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    assert itr == itr2
    print(f"{prec} {n}^3  pcg mgrb on a random problem: {itr} iterations, solve {t_solve * 1e3:.2f} ms; two imports + solve + export {t_all * 1e3:.2f} ms "
          f"(import + export: {(t_all - t_solve) / t_all * 100:.1f} %)", flush=True)
cz.close()
