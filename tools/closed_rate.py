"""What the closed box costs pcg (profiles/r17/closed.txt): `python tools/closed_rate.py [N] [PREC ...]` solves a seeded
problem `N N N pcg 1000 COEF PC` (default 512, f32 and f64; mg at 0.8 and mgrb at 1.2) in one process, on one handle and from the same start
field, first with five Neumann faces (Z+ stays Dirichlet) and then in the closed box, and prints one JSON line per leg: iterations, ms per
PCG iteration of three timed solves (their smallest, median and largest: the leg's own repeat spread), and from one more solve with
per-launch HIP events the launches and ms per launch of the labelled kernels.  The closed leg adds the modelled traffic of its own two
kernels: shift_sums moves 1 array (the pass that sums) or 2 (the pass that subtracts), 1.5 on average over the pairs it runs in; the closed
cg_update reads 4 arrays and writes 2.  ms per iteration is the solve's time over its iterations, so it carries the solve's two projections
(four shift_sums passes) and its first residual.

`python tools/closed_rate.py --unmasked LABEL [N]` is the other half of profiles/r17/closed.txt: the unmasked `N N N pcg 1000 0.8 jacobi` in
FP64 on the build of the checkout it is run from, three timed solves, one JSON line tagged LABEL.  Run it alternately from a built checkout of
the parent commit and from this one (A B A B, one process each) and append the lines."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cubez_amd import CZ  # noqa: E402
from cubez_amd.lib import LABELS  # noqa: E402

FIVE = [1, 1, 1, 1, 1, 0]
if len(sys.argv) > 2 and sys.argv[1] == "--unmasked":
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 512
    cz = CZ("f64", quiet=True)
    assert cz.setup([n, n, n, "pcg", 1000, 0.8, "jacobi"]) == 1
    start = cz.get_field()
    per = []
    for leg in range(4):
        cz.set_field(start)
        itr = cz.solve()
        assert itr > 0, "the solve broke down"
        if leg:
            per.append(round(1e3 * cz.solve_seconds / itr, 4))
    print(json.dumps(dict(build=sys.argv[2], itr=itr, res=cz.res, ms_per_itr=per, cg_fused=cz.info()["cg_fused"])), flush=True)
    cz.close()
    sys.exit(0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
precs = sys.argv[2:] or ["f32", "f64"]

for prec in precs:
    R = np.float32 if prec == "f32" else np.float64
    rng = np.random.default_rng(1000)
    b = ((rng.random((n, n, n), dtype=np.float32) * 2.0 - 1.0) * 1e-2).astype(R)
    start = rng.random((n, n, n), dtype=np.float32).astype(R)
    cells = float(n - 2) ** 3 * np.dtype(R).itemsize
    for pc, coef in (("mg", 0.8), ("mgrb", 1.2)):
        cz = CZ(prec, quiet=True)
        assert cz.setup([n, n, n, "pcg", 1000, coef, pc]) == 1
        for closed in (False, True):
            if closed:
                cz.set_closed_box(True)
            else:
                cz.set_neumann(FIVE)
            cz.set_rhs(b)
            out = dict(n=n, prec=prec, pc=pc, coef=coef, neumann=cz.info()["neumann"], closed=cz.info()["closed"])
            per = []
            for leg in range(5):
                cz.set_field(start)
                if leg == 4:
                    cz.timing(True)
                itr = cz.solve()
                assert itr > 0, f"{prec} {pc} closed={closed}: the solve broke down"
                if 1 <= leg <= 3:
                    per.append(1e3 * cz.solve_seconds / itr)
                    out.update(itr=itr, res=cz.res)
                if leg == 4:
                    t = {k: cz.timing_read(k) for k in LABELS}
                    cz.timing(False)
                    out["kernels"] = {k: [c, round(ms / c, 5)] for k, (c, ms) in t.items() if c > 0}
                    if closed:
                        out["means"] = [cz.closed_mean(w) for w in range(3)]
                        for k, arrays in (("shift_sums", 1.5), ("cg_update_closed", 6.0)):
                            c, ms = t[k]
                            out[k + "_TBps"] = round(arrays * cells * c / (ms * 1e-3) / 1e12, 3) if ms > 0 else None
            per.sort()
            out["ms_per_itr"] = [round(v, 4) for v in per]
            print(json.dumps(out), flush=True)
        cz.close()
