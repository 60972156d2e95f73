"""One leg of tests/test_gpu_switches.py: a fresh process whose environment holds the switch under test (the kernel context reads the
environment once per thread, the driver once per CZ, the communicator once per context -- so a leg cannot share a process with another).

    python switch_worker.py <outdir> <json: {"cases": [names of switch_table.CASES], "abi": bool}>

Runs every case through cubez_amd.CZ with the launch timing on and writes <outdir>/result.json (per case: iteration count, res, history,
launch count of every timing label, cz_info, cz_config_in_force, czhip_tuning_describe, wall time; czhip_config_describe(1) once) and
<outdir>/<case>.npy (the field; decomposed cases: the global field assembled from the bricks, ranks as threads over the LOCAL transport).
With "abi": also the C-ABI checks of test_gpu_kernels.py and test_gpu_pass_contract.py under the same environment, after the solves (their
clean-up restores setter defaults on the context)."""
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import switch_table as T  # noqa: E402


def case_args(c):
    """(prec, gsz, solver, itr_max, coef, pc, div) of a case"""
    if c["family"] == "krylov":
        m = importlib.import_module(c["module"])
        k = next(x for x in m.CASES if x["id"] == c["id"])
        itr_max = k["K"] + 1 if c["module"] == "bicg_parity" else k["K"]
        return k["prec"], tuple(k["gsz"]), k["solver"], itr_max, k["coef"], k["pc"], c["div"]
    return c["prec"], c["gsz"], c["solver"], c["itr_max"], c["coef"], c["pc"], c["div"]


def run_single(prec, gsz, solver, itr_max, coef, pc):
    from cubez_amd import CZ
    cz = CZ(prec, quiet=True)
    try:
        assert cz.setup(list(gsz) + [solver, itr_max, coef] + ([pc] if pc else [])) == 1
        cz.timing(True)
        itr = cz.solve()
        rec = dict(itr=itr, res=cz.res, history=list(cz.history()), launches=cz.launches(), info=cz.info(), in_force=cz.config_in_force(),
                   tuning=cz.tuning())
        cz.timing(False)
        P = cz.field()
        if solver in ("jacobi", "sor2sma"):
            # the export of the caller's-problem interface (CZ_FIELD_FORM): the owned brick [i, j, k] of the same field
            brick = cz.get_field()
            rec["info"]["field_form"] = cz.info()["field_form"]
            rec["get_field_equals_field"] = bool(np.array_equal(brick, np.transpose(P[2:-2, 2:-2, 2:-2], (1, 0, 2))))
        return rec, P
    finally:
        cz.close()


def run_decomposed(prec, gsz, solver, itr_max, coef, pc, div):
    from test_gpu_decomp import _decomposed
    results, G = _decomposed(prec, gsz, solver, itr_max, coef, div, pc=pc, overlap=int(os.environ.get("CZ_OVERLAP", "1")))
    ranks = [dict(itr=itr, res=res, history=list(hist), launches=loc["launches"], info=loc["info"], in_force=loc["in_force"], tuning=loc["tuning"])
             for itr, res, hist, P, loc in results]
    rec = dict(ranks[0], ranks=ranks)
    return rec, G


def abi_checks():
    """the drop-in symbols (res handed in non-zero: accumulation) and the checked single-sweep launches against the oracle, on their smallest
    boxes; returns how many ran"""
    import test_gpu_kernels as K
    import test_gpu_pass_contract as PC
    from oracle import cz_oracle as O
    n = 0
    boxes = [b for b in K.BOXES if b[0] in ((5, 4, 6), (24, 20, 28), (12, 10, 20), (130, 20, 252))]
    assert len(boxes) == 5
    for prec in ("f32", "f64"):
        for box in boxes:
            K.test_random_boxes_vs_oracle(prec, box)  # jacobi_ (res = 1.5 handed in), psor2sma_core_ (res carried over the colours), the rest
            n += 1
        for box in [b for b in K.MAF_BOXES if b[0] in ((9, 12, 7), (24, 20, 28))]:
            K.test_maf_random_boxes_vs_oracle(prec, box)
            # jacobi_maf_ with a non-zero res handed in
            (ni, nj, nk), idx = box
            sz, idx = [ni, nj, nk], list(idx) if idx else [2, ni - 1, 2, nj - 1, 2, nk - 1]
            h, ko = K._hip(prec), O.Kernels("oracle", prec)
            rng = np.random.default_rng(ni + nj + nk)
            xc, yc, zc = (K._coords(rng, m, ko.real) for m in (ni, nj, nk))
            p, b = (rng.uniform(-1, 1, (nj + 4, ni + 4, nk + 4)).astype(ko.real) for _ in range(2))
            a1, w1, wide = p.copy(), np.zeros_like(p), np.zeros(1)
            ko.jacobi_maf(a1, sz, idx, xc, yc, zc, 0.9, b, w1, res=0.0, wide=wide)
            a2, w2, db = h.alloc(sz, p), h.alloc(sz, np.zeros_like(p)), h.alloc(sz, b)
            r2 = h.jacobi_maf(a2, sz, idx, xc, yc, zc, 0.9, db, w2, res=2.5)
            assert K._beq(a2.get(), a1) and K._rel(r2 - 2.5, wide[0]) < K.RTOL_WIDE * 10, (prec, box, r2, wide[0])
            for a in (a2, w2, db):
                a.free()
            n += 1
        for kind in ("jacobi", "rbsor"):
            for box in PC.BOXES:
                PC.test_checked_launch_bookkeeping_against_wide_oracle(kind, box, prec)
                PC.test_launch_after_convergence_changes_nothing(kind, box, prec)
                n += 2
    return n


def main():
    outdir, job = sys.argv[1], json.loads(sys.argv[2])
    from cubez_amd import load
    lib = load("f32")
    lib.czhip_config_describe.restype = C.c_char_p
    out = dict(config_set=lib.czhip_config_describe(1).decode(), cases={})
    for name in job["cases"]:
        prec, gsz, solver, itr_max, coef, pc, div = case_args(T.CASES[name])
        t0 = time.time()
        rec, P = run_decomposed(prec, gsz, solver, itr_max, coef, pc, div) if div else run_single(prec, gsz, solver, itr_max, coef, pc)
        rec["wall_s"] = time.time() - t0
        np.save(os.path.join(outdir, name + ".npy"), P)
        out["cases"][name] = rec
    if job.get("abi"):
        t0 = time.time()
        out["abi"] = dict(ran=abi_checks(), wall_s=time.time() - t0)
    with open(os.path.join(outdir, "result.json.tmp"), "w") as f:
        json.dump(out, f)
    os.rename(os.path.join(outdir, "result.json.tmp"), os.path.join(outdir, "result.json"))


if __name__ == "__main__":
    main()
