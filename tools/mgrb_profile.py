"""One leg of the pcg mg / mgrb comparison (profiles/r12/mgrb.txt): `python tools/mgrb_profile.py ROOT PREC N PC COEF` imports cubez_amd from
the tree at ROOT, solves `N N N pcg 1000 COEF PC` twice and prints one JSON line for the second solve: iterations, seconds to convergence,
ms per PCG iteration, and (from a third solve with per-launch HIP events) ms per launch of the labelled multigrid kernels."""
import ctypes as C
import json
import os
import sys

root, prec, n, pc, coef = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4], float(sys.argv[5])
sys.path.insert(0, root)
from cubez_amd import CZ  # noqa: E402

out = dict(root=root, prec=prec, n=n, pc=pc, coef=coef, env={k: os.environ[k] for k in ("CZ_MGRB_ZERO4", "CZHIP_RB4") if k in os.environ})
for leg in range(3):
    cz = CZ(prec, quiet=True)
    cz.lib.cz_last_solve_seconds.restype = C.c_double
    cz.lib.cz_last_solve_seconds.argtypes = [C.c_void_p]
    assert cz.setup([n, n, n, "pcg", 1000, coef, pc]) == 1
    if leg == 2:
        cz.timing(True)
    itr = cz.solve()
    s = cz.lib.cz_last_solve_seconds(cz.h)
    if leg == 1:
        out.update(itr=itr, seconds=round(s, 6), ms_per_itr=round(1e3 * s / itr, 4))
    if leg == 2:
        for label in ("mg_rb", "mg_smooth", "mg_restrict", "mg_prolong", "mg_tail", "rbsor4", "rbsor2", "jacobi2"):
            cnt, ms = cz.timing_read(label)
            if cnt > 0:
                out[label] = [cnt, round(ms / cnt, 5)]
        cz.timing(False)
    cz.close()
print(json.dumps(out), flush=True)
