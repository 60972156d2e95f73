"""python3 tools/mg_cycle_rate.py ROOT [n=512] [reps=21]: per precision and preconditioner (constant weights), one V-cycle per cz_precondition from the tree at ROOT (its directory name leads every line):
ms per cycle under each multigrid label, median (min, max) over the repeats after 3 warm-up calls.  With `coef`: the same under coefficients."""
import os
import statistics
import sys

import numpy as np

root = sys.argv[1]
sys.path.insert(0, root)
from cubez_amd import CZ  # noqa: E402

n = int(sys.argv[2]) if len(sys.argv) > 2 else 512
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 21
labels = ("mg_tail", "mg_smooth", "mg_rb", "mg_restrict")
for prec, R in (("f32", np.float32), ("f64", np.float64)):
    rng = np.random.default_rng(1000)
    rpad = np.zeros((n + 4, n + 4, n + 4), dtype=R)
    rpad[3:-3, 3:-3, 3:-3] = rng.standard_normal((n - 2, n - 2, n - 2)).astype(R)
    ones = [np.ones((n, n, n), dtype=R) for _ in range(3)]
    for coef_on in (False, True):
        for pc, om in (("mg", 0.8), ("mgrb", 1.2)):
            cz = CZ(prec, quiet=True)
            assert cz.setup([n, n, n, "pcg", 1, om, pc]) == 1
            if coef_on:
                cz.set_face_coef(*ones)
                cz.set_coef_mg(True)
                assert cz.info()["coef_mg"] == 1
            cz.timing(True)
            for _ in range(3):
                cz.precondition(rpad)
            out = {k: [] for k in labels}
            for _ in range(reps):
                t0 = {k: cz.timing_read(k) for k in labels}
                cz.precondition(rpad)
                for k in labels:
                    c1, t1 = cz.timing_read(k)
                    if c1 > t0[k][0]:
                        out[k].append(t1 - t0[k][1])
            cz.timing(False)
            cz.close()
            for k in labels:
                if out[k]:
                    print(f"{os.path.basename(os.path.abspath(root))} {prec} {n}^3 {'coef ' if coef_on else 'const'} {pc:4s} {k:11s}: median {statistics.median(out[k]):.5f} ms per cycle "
                          f"(min {min(out[k]):.5f}, max {max(out[k]):.5f})", flush=True)
