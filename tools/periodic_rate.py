"""What periodic directions cost pcg (profiles/r18/periodic.txt): `python tools/periodic_rate.py [N] [PREC ...]` solves a
seeded problem (tools/closed_rate.py's right-hand side and start field: the built-in one has b = 0 and its data on the Z faces, which a
periodic Z replaces) with `N N N pcg 1000 COEF PC` (default 512, f32 and f64; mg at 0.8 and mgrb at 1.2) in one process and on one handle,
from the same start field, in three legs: no flag, periodic X, and the channel (the closed box with periodic X and Z, walls in Y), and prints one JSON
line per leg: iterations, ms per PCG iteration (the second of two solves), and from a third solve with per-launch HIP events the launches
and ms per launch of the labelled kernels and the fills' share of the labelled time (they run under the label bc_mirror)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cubez_amd import CZ  # noqa: E402
from cubez_amd.lib import LABELS  # noqa: E402

LEGS = (("none", False, (0, 0, 0)), ("periodic_x", False, (1, 0, 0)), ("channel", True, (1, 0, 1)))
n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
precs = sys.argv[2:] or ["f32", "f64"]

for prec in precs:
    R = np.float32 if prec == "f32" else np.float64
    rng = np.random.default_rng(1000)
    b = ((rng.random((n, n, n), dtype=np.float32) * 2.0 - 1.0) * 1e-2).astype(R)
    start = rng.random((n, n, n), dtype=np.float32).astype(R)
    for pc, coef in (("mg", 0.8), ("mgrb", 1.2)):
        cz = CZ(prec, quiet=True)
        assert cz.setup([n, n, n, "pcg", 1000, coef, pc]) == 1
        cz.set_rhs(b)
        for name, closed, per in LEGS:
            if closed:
                cz.set_closed_box(True)
            cz.set_periodic(per)
            if closed:
                cz.set_rhs(b)  # (the closed mode projected the handle's copy: every leg starts from the same b)
            info = cz.info()
            out = dict(n=n, prec=prec, pc=pc, coef=coef, leg=name, periodic=info["periodic"], closed=info["closed"])
            for leg in range(3):
                cz.set_field(start)
                if leg == 2:
                    cz.timing(True)
                itr = cz.solve()
                if leg == 1:
                    out.update(itr=itr, res=cz.res, ms_per_itr=round(1e3 * cz.solve_seconds / itr, 4))
                if leg == 2:
                    t = {k: cz.timing_read(k) for k in LABELS}
                    cz.timing(False)
                    total = sum(ms for _, ms in t.values())
                    out["kernels"] = {k: [c, round(ms / c, 5)] for k, (c, ms) in t.items() if c > 0}
                    out["fill_share"] = round(t["bc_mirror"][1] / total, 5) if total > 0 else 0.0
            print(json.dumps(out), flush=True)
        cz.close()
