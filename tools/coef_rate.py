"""The face-coefficient kernels (cz_set_face_coef) against a device-to-device copy of the bytes each one moves, and what the
variable operator costs a solve:
    python3 tools/coef_rate.py [n=512] [repeats=11]
Per precision, C order, in one process.  Kernels: median time over the repeats after 3 warm-up calls, by the library's HIP events under the
label each launch runs under -- the SpMV with its two dots (calc_ax: 4 reads + 1 write = 5 array passes) and the residual (calc_rk: 5 + 1 = 6)
from one-iteration solves of `pcg none`, the gradient (field_io: 4 reads + 3 read-modify-writes = 10) from sub_grad, the scaling (ewise:
2 reads + 1 write = 3) from one-iteration solves of `pcg jacobi`; hipMemcpyDtoDAsync moving the same bytes, timed with events on one stream.
Solves: `pcg mg 0.8` and `pcg mgrb 1.2` on a seeded problem to eps 1e-5 with smooth(4) coefficients and without any: iterations and ms per
iteration (wall time of cz_solve over its iterations, the median of the repeats)."""
import ctypes as C
import math
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


def label_ms(cz, fn, labels):
    """{label: (median, min, max)} of the time per launch of fn()'s launches under each label over the repeats"""
    for _ in range(3):
        fn()
    out = {k: [] for k in labels}
    for _ in range(reps):
        before = {k: cz.timing_read(k) for k in labels}
        fn()
        cz.lib.czhip_sync()
        for k in labels:
            n1, t1 = cz.timing_read(k)
            assert n1 - before[k][0] == labels[k], (k, n1 - before[k][0], labels[k])
            out[k].append((t1 - before[k][1]) / labels[k])
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def event_ms(s, fn):
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


def smooth(dt, ratio):
    """tests/coef_parity.smooth on the device: ratio ** (a product of three sines scaled to [0, 1]) at the face centres"""
    out = []
    for ax in range(3):
        pts = []
        for d in range(3):
            c = (torch.arange(n, dtype=torch.float64, device="cuda") + (0.5 if d == ax else 0.0)) / (n - 1.0)
            pts.append(c.reshape([-1 if q == d else 1 for q in range(3)]))
        f = 0.5 * (1.0 + torch.sin(2.0 * math.pi * pts[0]) * torch.sin(2.0 * math.pi * pts[1]) * torch.sin(2.0 * math.pi * pts[2]))
        out.append((float(ratio) ** f).to(dt).contiguous())
    return out


def report(prec, what, passes, t, copy, cells, esz):
    med, lo, hi = t
    print(f"{prec} {n}^3  {what:22s}: median {med:.4f} ms (min {lo:.4f}, max {hi:.4f})  {passes * cells * esz / med / 1e6:.0f} GB/s over {passes} array passes"
          f"  = {med / copy[passes]:.2f} x the copy of its bytes", flush=True)


for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
    esz = 4 if prec == "f32" else 8
    cells = n ** 3
    s = torch.cuda.Stream()
    torch.manual_seed(1000)
    b = (torch.rand((n, n, n), dtype=dt, device="cuda") * 2.0 - 1.0) * 1e-2
    p = torch.rand((n, n, n), dtype=dt, device="cuda")
    u, v, w = (torch.rand((n, n, n), dtype=dt, device="cuda") for _ in range(3))
    beta = smooth(dt, 4)
    torch.cuda.synchronize()
    copy = {}
    for passes in (3, 5, 6, 10):  # a copy reads and writes: `passes` array passes are passes / 2 array copies
        nbytes = passes * cells * esz // 2
        src, dst = torch.ones(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        med, lo, hi = event_ms(s, lambda: hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), nbytes, s.cuda_stream))
        copy[passes] = med
        print(f"{prec} {n}^3  hipMemcpyDtoDAsync of {passes} array passes ({2 * nbytes / 1e9:.3f} GB moved): median {med:.4f} ms (min {lo:.4f}, max {hi:.4f})  "
              f"{2 * nbytes / med / 1e6:.0f} GB/s", flush=True)
        del src, dst
    # -- the kernels, one launch each per one-iteration solve
    for pc in ("none", "jacobi"):
        cz = CZ(prec, quiet=True)
        assert cz.setup([n, n, n, "pcg", 1, 0.8, pc]) == 1
        cz.timing(True)
        cz.set_eps(1e-30)
        cz.set_rhs(b)
        cz.set_field(p)
        cz.set_face_coef(*beta)
        if pc == "none":
            t = label_ms(cz, cz.solve, {"calc_ax": 1, "calc_rk": 1})
            report(prec, "SpMV + p.q, q.q", 5, t["calc_ax"], copy, cells, esz)
            report(prec, "residual + sum r^2", 6, t["calc_rk"], copy, cells, esz)
            with torch.cuda.stream(s):
                t = label_ms(cz, lambda: cz.sub_grad(u, v, w, 1e-3), {"field_io": 1})
            report(prec, f"sub_grad (form {cz.info()['field_form']})", 10, t["field_io"], copy, cells, esz)
        else:
            # ewise also holds the direction's copy-free updates of the iteration: take the scaling alone as the difference to a handle without
            # coefficients
            def ewise_total():
                n0, t0 = cz.timing_read("ewise")
                cz.solve()
                cz.lib.czhip_sync()
                n1, t1 = cz.timing_read("ewise")
                return n1 - n0, t1 - t0
            for _ in range(3):
                ewise_total()
            with_coef = [ewise_total() for _ in range(reps)]
            cz.set_face_coef(None)
            for _ in range(3):
                ewise_total()
            without = [ewise_total() for _ in range(reps)]
            extra = with_coef[0][0] - without[0][0]
            d = statistics.median(a[1] for a in with_coef) - statistics.median(a[1] for a in without)
            print(f"{prec} {n}^3  scaling out = s in: {extra} more ewise launches per iteration, {d / max(extra, 1):.4f} ms each by the difference of the medians"
                  f"  = {d / max(extra, 1) / copy[3]:.2f} x the copy of its bytes", flush=True)
        cz.close()
    # -- the solves
    for pc, coef in (("mg", 0.8), ("mgrb", 1.2)):
        cz = CZ(prec, quiet=True)
        assert cz.setup([n, n, n, "pcg", 300, coef, pc]) == 1
        cz.set_eps(1e-5)
        cz.set_rhs(b)
        for name, bt in (("no coefficients", None), ("smooth(4)", beta)):
            if bt is not None:
                cz.set_face_coef(*bt)
            per, its = [], 0
            for r in range(3 + reps):
                cz.set_field(p)
                its = cz.solve()
                if r >= 3:
                    per.append(cz.solve_seconds * 1e3 / max(its, 1))
            print(f"{prec} {n}^3  pcg {pc} {coef}, {name:15s}: {its} iterations to eps 1e-5 (cg_fused {cz.info()['cg_fused']}), median {statistics.median(per):.3f} ms per iteration"
                  f" (min {min(per):.3f}, max {max(per):.3f})", flush=True)
        cz.close()
    del b, p, u, v, w, beta
    torch.cuda.empty_cache()
