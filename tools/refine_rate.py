"""Mixed-precision refinement (cubez_amd.Refined) against the FP64 library alone, to a true relative residual <= 1e-10:
    python3 tools/refine_rate.py [n=512] [rounds=3]
One process, single domain, the legs interleaved A B A B ...:
    A  FP64 pcg 1000 1.2 mgrb on a random problem, set_eps tightened (x 0.1 from 1e-6) until cz_get_residual says |b - A p| <= 1e-10 |b - A p0|;
       the time is that of the solves alone (wall clock around cz.solve, the device idle before and after), summed over the tightening steps
    B  Refined to the same bar (wall clock around Refined.solve)
Per leg: every round's time, the median and the spread (min, max).  Then the fused residual pass alone (HIP events, label field_io; FP64 handle,
float32 and float64 destinations, and the norm only) against hipMemcpyDtoDAsync of one padded FP64 array in the same process."""
import ctypes as C
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cubez_amd import CZ, Refined  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
TOL = 1e-10
gsz = (n, n, n)
torch.manual_seed(1)
b = (torch.rand(gsz, dtype=torch.float64, device="cuda") * 2 - 1) * 1e-2
p0 = torch.rand(gsz, dtype=torch.float64, device="cuda")

a64 = CZ("f64", quiet=True)
assert a64.setup(list(gsz) + ["pcg", 1000, 1.2, "mgrb"]) == 1
rf = Refined(gsz)


def leg_a():
    a64.set_rhs(b)
    a64.set_field(p0)
    _, s0 = a64.get_residual()
    eps, t, iters = 1e-6, 0.0, 0
    while True:
        a64.set_eps(eps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it = a64.solve()
        torch.cuda.synchronize()
        t += time.perf_counter() - t0
        assert it > 0
        iters += it
        _, s = a64.get_residual()
        if math.sqrt(s) <= TOL * math.sqrt(s0):
            return t, iters, math.sqrt(s / s0), eps
        eps *= 0.1


def leg_b():
    rf.set_rhs(b)
    rf.set_field(p0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    k = rf.solve(tol=TOL)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    assert k > 0
    return t, rf.history


ta, tb = [], []
for r in range(rounds + 1):  # (round 0 warms both legs up and is not counted)
    t, iters, rel, eps = leg_a()
    if r:
        ta.append(t)
    print(f"round {r} A  FP64 pcg mgrb {n}^3: {t * 1e3:.2f} ms, {iters} iterations, eps {eps:g}, true relative residual {rel:.3g}", flush=True)
    t, hist = leg_b()
    if r:
        tb.append(t)
    print(f"round {r} B  Refined      {n}^3: {t * 1e3:.2f} ms, {len(hist)} outer steps, inner iterations {[h[2] for h in hist]}, true relative residual {hist[-1][1]:.3g}",
          flush=True)
ma, mb = statistics.median(ta), statistics.median(tb)
print(f"A median {ma * 1e3:.2f} ms (min {min(ta) * 1e3:.2f}, max {max(ta) * 1e3:.2f});  B median {mb * 1e3:.2f} ms (min {min(tb) * 1e3:.2f}, max {max(tb) * 1e3:.2f});  "
      f"A / B = {ma / mb:.3f}", flush=True)

# the fused residual pass alone
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
cz, reps = rf.hi, 11
cz.timing(True)
s = torch.cuda.Stream()
pad_elems = (n + 4) ** 3
src, dst = torch.ones(pad_elems, dtype=torch.float64, device="cuda"), torch.empty(pad_elems, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
times = []
for r in range(3 + reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    assert hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), pad_elems * 8, s.cuda_stream) == 0
    e1.record(s)
    s.synchronize()
    if r >= 3:
        times.append(e0.elapsed_time(e1))
cp = statistics.median(times)
print(f"hipMemcpyDtoDAsync of one padded FP64 array: median {cp:.4f} ms (min {min(times):.4f}, max {max(times):.4f})  {16 * pad_elems / cp / 1e6:.0f} GB/s", flush=True)
del src, dst
with torch.cuda.stream(s):
    for name, out, nbytes in (("float32 destination", torch.empty(gsz, dtype=torch.float32, device="cuda"), 20), ("float64 destination", torch.empty(gsz, dtype=torch.float64, device="cuda"), 24),
                              ("norm only", None, 16)):
        t = []
        for r in range(3 + reps):
            n0, t0 = cz.timing_read("field_io")
            cz.get_residual(out=out, scale=2.0 ** 9)
            n1, t1 = cz.timing_read("field_io")
            assert n1 - n0 == 1
            if r >= 3:
                t.append(t1 - t0)
        med = statistics.median(t)
        print(f"fused residual pass, FP64 handle, {name:20s}: median {med:.4f} ms (min {min(t):.4f}, max {max(t):.4f})  {nbytes * n ** 3 / med / 1e6:.0f} GB/s "
              f"of {nbytes} B per cell = {med / cp:.2f} x the copy", flush=True)
rf.close()
a64.close()
