"""Which kernels the Krylov loops launch, and how often (profiles/r30/pcg_launches_*.txt): a refactor of the host driver must leave the
table as it was.

    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python3 tools/pcg_launch_counts.py PREC
    python3 tools/pcg_launch_counts.py --table OUT

The first form runs, in one process and on the build of the checkout it is run from, small solves on a 33 x 47 x 61 box cut at five
iterations (eps 1e-30), PREC = f32 | f64 (two libraries, hence two invocations): pcg none | jacobi | mg | mgrb; jacobi with one Neumann
face and with one periodic direction; mgrb on the closed box; mg with face coefficients, without and with cz_set_coef_mg; jacobi and
mgrb again with CZ_CG_FUSE=0; pbicgstab jacobi and sor2sma with CZ_BICG_DEVSC on and off.  It prints one line per solve (iterations,
last residual), which must not move either.  No counters in that run.  The second form prints `calls  kernel` from the profiler's own
kernel statistics under OUT, sorted by name: two such tables are compared with diff."""
import csv
import glob
import os
import sys

GSZ = (33, 47, 61)


def table(out):
    files = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        sys.exit(f"no *kernel_stats.csv under {out}")
    calls = {}
    for f in files:
        with open(f, newline="") as fp:
            for row in csv.DictReader(fp):
                name = row.get("Name") or row.get("KernelName") or row["Kernel_Name"]
                calls[name] = calls.get(name, 0) + int(row.get("Calls") or row["Count"])
    for name in sorted(calls):
        print(f"{calls[name]:7d}  {name}")
    print(f"{sum(calls.values()):7d}  launches of {len(calls)} kernels")


def solves(prec):
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from cubez_amd import CZ
    R = np.float32 if prec == "f32" else np.float64
    rng = np.random.default_rng(30)
    b = ((rng.random(GSZ) * 2.0 - 1.0) * 1e-2).astype(R)
    start = rng.random(GSZ).astype(R)
    beta = [(1.0 + rng.random(GSZ)).astype(R) for _ in range(3)]

    def run(tag, solver, coef, pc, env=None, prepare=None):
        for k, v in (env or {}).items():
            os.environ[k] = v  # (a handle reads the driver's switches when it is made)
        cz = CZ(prec, quiet=True)
        try:
            assert cz.setup(list(GSZ) + [solver, 5, coef, pc]) == 1
            if prepare:
                prepare(cz)
            cz.set_rhs(b)
            cz.set_field(start)
            cz.set_eps(1e-30)
            itr = cz.solve()
            assert itr > 0, f"{tag}: the solve failed"
            print(f"{prec} {tag}: itr {itr} res {cz.res!r}", flush=True)
        finally:
            cz.close()
            for k in env or {}:
                del os.environ[k]

    def coefs(mg):
        def prepare(cz):
            cz.set_face_coef(*beta)
            cz.set_coef_mg(mg)
        return prepare

    for pc, coef in (("none", 1.0), ("jacobi", 0.8), ("mg", 0.8), ("mgrb", 1.2)):
        run(f"pcg {pc}", "pcg", coef, pc)
    run("pcg jacobi, one Neumann face", "pcg", 0.8, "jacobi", prepare=lambda cz: cz.set_neumann([1, 0, 0, 0, 0, 0]))
    run("pcg jacobi, one periodic direction", "pcg", 0.8, "jacobi", prepare=lambda cz: cz.set_periodic([0, 0, 1]))
    run("pcg mgrb, closed box", "pcg", 1.2, "mgrb", prepare=lambda cz: cz.set_closed_box(True))
    run("pcg mg, face coefficients", "pcg", 0.8, "mg", prepare=coefs(False))
    run("pcg mg, face coefficients, cz_set_coef_mg", "pcg", 0.8, "mg", prepare=coefs(True))
    run("pcg jacobi, CZ_CG_FUSE=0", "pcg", 0.8, "jacobi", env={"CZ_CG_FUSE": "0"})
    run("pcg mgrb, CZ_CG_FUSE=0", "pcg", 1.2, "mgrb", env={"CZ_CG_FUSE": "0"})
    for pc, coef in (("jacobi", 0.8), ("sor2sma", 1.5)):
        for devsc in ("1", "0"):
            run(f"pbicgstab {pc}, CZ_BICG_DEVSC={devsc}", "pbicgstab", coef, pc, env={"CZ_BICG_DEVSC": devsc})


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--table":
        table(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] in ("f32", "f64"):
        solves(sys.argv[1])
    else:
        sys.exit(__doc__)
