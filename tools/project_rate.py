"""The projection kernels (cz_set_rhs_div, cz_sub_grad) against the torch-slice composition they replace and against a
device-to-device copy of the same bytes:
    python3 tools/project_rate.py [n=512] [repeats=11]
Per precision, C order, in one process: median kernel time over the repeats (HIP events around the launch, label field_io) after 3 warm-up
calls of set_rhs_div (3 reads + 1 write = 4 array passes) and sub_grad (1 read + 3 read-modify-writes = 7 array passes);
hipMemcpyDtoDAsync moving the same bytes (2 and 3.5 array copies) timed with events on the same stream; the torch-slice divergence and
gradient of the Level-3 loop of before (the arithmetic on the inner cells only, events on torch's stream), with the whole-array trips
set_rhs(b) and get_field(p) that went with them."""
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cubez_amd import CZ  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 11
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]


def label_ms(cz, fn, launches=1):
    """median time of fn()'s field_io launches over the repeats"""
    for _ in range(3):
        fn()
    out = []
    for _ in range(reps):
        n0, t0 = cz.timing_read("field_io")
        fn()
        cz.lib.czhip_sync()
        n1, t1 = cz.timing_read("field_io")
        assert n1 - n0 == launches, (n1 - n0, launches)
        out.append(t1 - t0)
    return statistics.median(out), min(out), max(out)


def event_ms(s, fn):
    """median time of fn() on stream s over the repeats, by events"""
    out = []
    for r in range(3 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        s.synchronize()
        if r >= 3:
            out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def torch_div(u, v, w):
    """the Level-3 loop's divergence on the inner cells (Dirichlet box), written with slices"""
    b = torch.zeros_like(u)
    b[1:-1, 1:-1, 1:-1] = ((u[1:-1, 1:-1, 1:-1] - u[:-2, 1:-1, 1:-1]) + (v[1:-1, 1:-1, 1:-1] - v[1:-1, :-2, 1:-1])) + (w[1:-1, 1:-1, 1:-1] - w[1:-1, 1:-1, :-2])
    return b


def torch_grad(u, v, w, p):
    u[:-1, 1:-1, 1:-1] -= p[1:, 1:-1, 1:-1] - p[:-1, 1:-1, 1:-1]
    v[1:-1, :-1, 1:-1] -= p[1:-1, 1:, 1:-1] - p[1:-1, :-1, 1:-1]
    w[1:-1, 1:-1, :-1] -= p[1:-1, 1:-1, 1:] - p[1:-1, 1:-1, :-1]


for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
    esz = 4 if prec == "f32" else 8
    cells = n ** 3
    cz = CZ(prec, quiet=True)
    assert cz.setup([n, n, n, "pcg", 10, 1.2, "mgrb"]) == 1
    cz.timing(True)
    s = torch.cuda.Stream()
    u, v, w, p = (torch.rand((n, n, n), dtype=dt, device="cuda") for _ in range(4))
    cz.set_field(p)
    torch.cuda.synchronize()
    copy = {}
    for passes in (4, 7):  # a copy reads and writes: `passes` array passes are passes / 2 array copies
        nbytes = passes * cells * esz // 2
        src, dst = torch.ones(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        med, lo, hi = event_ms(s, lambda: hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), nbytes, s.cuda_stream))
        copy[passes] = med
        print(f"{prec} {n}^3  hipMemcpyDtoDAsync of {passes} array passes ({2 * nbytes / 1e9:.3f} GB moved): median {med:.4f} ms (min {lo:.4f}, max {hi:.4f})  "
              f"{2 * nbytes / med / 1e6:.0f} GB/s", flush=True)
        del src, dst
    with torch.cuda.stream(s):
        for what, passes, fn in (("set_rhs_div", 4, lambda: cz.set_rhs_div(u, v, w, want_norm=False)), ("sub_grad", 7, lambda: cz.sub_grad(u, v, w, 1e-3))):
            med, lo, hi = label_ms(cz, fn)
            print(f"{prec} {n}^3  {what:11s} (form {cz.info()['field_form']}): median {med:.4f} ms (min {lo:.4f}, max {hi:.4f})  "
                  f"{passes * cells * esz / med / 1e6:.0f} GB/s over {passes} array passes  = {med / copy[passes]:.2f} x the copy of its bytes", flush=True)
        for what, fn in (("torch slices: divergence", lambda: torch_div(u, v, w)), ("torch slices: gradient", lambda: torch_grad(u, v, w, p))):
            med, lo, hi = event_ms(s, fn)
            print(f"{prec} {n}^3  {what:26s}: median {med:.4f} ms (min {lo:.4f}, max {hi:.4f})", flush=True)
        b = torch_div(u, v, w)
        med, lo, hi = label_ms(cz, lambda: cz.set_rhs(b))
        print(f"{prec} {n}^3  the trip that went with it, set_rhs(b): median {med:.4f} ms (min {lo:.4f}, max {hi:.4f})", flush=True)
        med, lo, hi = label_ms(cz, lambda: cz.get_field(p))
        print(f"{prec} {n}^3  the trip that went with it, get_field(p): median {med:.4f} ms (min {lo:.4f}, max {hi:.4f})", flush=True)
    cz.close()
    del u, v, w, p, b
    torch.cuda.empty_cache()
