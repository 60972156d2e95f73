"""What zero-flux (Neumann) faces cost pcg (profiles/r16/neumann.txt): `python tools/neumann_rate.py [N] [PREC ...]` solves the
built-in problem `N N N pcg 1000 COEF PC` (default 512, f32 and f64; mg at 0.8 and mgrb at 1.2) in one process, first with Dirichlet faces and
then, on the same handle and from the same start field, with five Neumann faces (Z+ stays Dirichlet), and prints one JSON line per leg:
iterations, ms per PCG iteration (the second of two solves), and from a third solve with per-launch HIP events the launches and ms per launch
of the labelled kernels and the mirror's share of the labelled time."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cubez_amd import CZ  # noqa: E402
from cubez_amd.lib import LABELS  # noqa: E402

FIVE = [1, 1, 1, 1, 1, 0]
n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
precs = sys.argv[2:] or ["f32", "f64"]

for prec in precs:
    for pc, coef in (("mg", 0.8), ("mgrb", 1.2)):
        cz = CZ(prec, quiet=True)
        assert cz.setup([n, n, n, "pcg", 1000, coef, pc]) == 1
        start = cz.get_field()
        for mask in ([0] * 6, FIVE):
            cz.set_neumann(mask)
            out = dict(n=n, prec=prec, pc=pc, coef=coef, neumann=cz.info()["neumann"])
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
                    out["mirror_share"] = round(t["bc_mirror"][1] / total, 5) if total > 0 else 0.0
            print(json.dumps(out), flush=True)
        cz.close()
