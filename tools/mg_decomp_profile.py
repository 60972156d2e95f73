"""Timings of `pcg ... mg` for profiles/r09/mg_decomp.txt: single-domain ms per iteration, and one distributed V-cycle of
two RCCL ranks that share ONE GPU (processes with their own host id, as tests/test_gpu_rccl.py), with the exchanges per V-cycle and a model of
the bytes each level sends.

    python tools/mg_decomp_profile.py                 # everything; prints the record
    python tools/mg_decomp_profile.py rank R W DIR N  # (internal) one rank of the two-rank V-cycle run

Two ranks on one GPU share its CUs and HBM and talk over RCCL's socket transport on the loopback interface: the numbers say nothing about
scaling across devices."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS = 20


def rank_main(rank, world, outdir, n):
    import numpy as np
    from cubez_amd import CZ, load
    lib = load("f64")
    assert lib.czhip_init(0) == 0
    buf = C.create_string_buffer(lib.cz_comm_unique_id_bytes())
    idf = os.path.join(outdir, "id")
    if rank == 0:
        lib.cz_comm_get_unique_id(buf)
        with open(idf + ".tmp", "wb") as f:
            f.write(buf.raw)
        os.rename(idf + ".tmp", idf)
    else:
        t0 = time.time()
        while not os.path.exists(idf):
            assert time.time() - t0 < 120, "no communicator id"
            time.sleep(0.05)
        buf.raw = open(idf, "rb").read()
    lib.cz_comm_bootstrap(rank, world, buf.raw)
    cz = CZ("f64", quiet=True, device=0)
    assert cz.setup([n, n, n, "pcg", 1000, 0.8, "mg", 2, 1, 1]) == 1
    r = np.random.default_rng(rank).standard_normal(cz.field().shape)
    cz.precondition(r)  # warm-up
    t0 = time.perf_counter()
    for _ in range(REPS):
        cz.precondition(r)
    t_cycle = (time.perf_counter() - t0) / REPS
    # the host copies inside cz_precondition (r up, z down), timed alone
    t0 = time.perf_counter()
    for _ in range(REPS):
        cz.field()
    t_d2h = (time.perf_counter() - t0) / REPS
    info = cz.info()
    # a whole solve for the time per PCG iteration
    itr = cz.solve()
    rec = dict(rank=rank, t_cycle_s=t_cycle, t_d2h_s=t_d2h, itr=itr, solve_s=cz.lib.cz_last_solve_seconds(cz.h), info=info, local=cz.local())
    with open(os.path.join(outdir, f"rank_{rank}.json"), "w") as f:
        json.dump(rec, f)
    cz.close()
    lib.cz_comm_shutdown()


def single(n, pc, itmax, prec="f64"):
    from cubez_amd import CZ
    out = []
    for _ in range(2):  # the second solve is reported (the first one pays the launches' first-use costs)
        cz = CZ(prec, quiet=True)
        assert cz.setup([n, n, n, "pcg", itmax, 0.8, pc]) == 1
        itr = cz.solve()
        out.append((itr, cz.lib.cz_last_solve_seconds(cz.h)))
        cz.close()
    return out[-1]


def level_kernels(n, prec):
    """HIP-event time of the level kernels over one solve: label -> (launches, ms per launch)"""
    from cubez_amd import CZ
    cz = CZ(prec, quiet=True)
    assert cz.setup([n, n, n, "pcg", 1000, 0.8, "mg"]) == 1
    cz.solve()
    cz.timing(True)
    cz.solve()
    out = {k: cz.timing_read(k) for k in ("mg_smooth", "mg_restrict", "mg_prolong", "mg_tail")}
    cz.timing(False)
    cz.close()
    return {k: (c, ms / max(c, 1)) for k, (c, ms) in out.items()}


def bytes_model(n, div, rank):
    """elements one brick sends per exchange at every distributed level: face exchange (owned face layers) and the face + edge + corner
    exchange; J faces travel as whole padded planes in the real exchange (a little more)"""
    from cubez_amd import decomp as D
    h, m = D.mg_points((n, n, n), div, rank)
    d = D.decompose((n, n, n), div, div[0] * div[1] * div[2], rank)
    G = D.mg_gather_level((n, n, n), div)
    rows = []
    for lev in range(max(G, 1)):
        c = [D.mg_own(h[a], m[a], lev)[1] for a in range(3)]
        nb = [(d["nID"][2 * a] >= 0, d["nID"][2 * a + 1] >= 0) for a in range(3)]
        face = sum((c[1] * c[2], c[0] * c[2], c[0] * c[1])[a] * (nb[a][0] + nb[a][1]) for a in range(3))
        full = face  # + edges and corners: with one cut direction there are none
        rows.append((lev, tuple(c), face * 8, full * 8))
    return G, rows


def main():
    from test_gpu_rccl import rank_env
    lines = []
    P = lines.append
    P("single domain, coefficient 0.8, eps 1e-5 (second of two solves, cz_last_solve_seconds)")
    for n, itmax in ((128, 1000), (512, 1000)):
        for pc, prec in (("mg", "f64"), ("jacobi", "f64"), ("mg", "f32")):
            itr, s = single(n, pc, itmax if pc == "mg" or n == 128 else 40, prec)
            P(f"  {n}^3 {prec} pcg {pc:6s}: {itr:4d} iterations{' (ItrMax 40)' if pc == 'jacobi' and n == 512 else ''}  {s * 1e3:9.2f} ms  "
              f"{s / itr * 1e3:8.3f} ms/iteration")
    for prec in ("f64", "f32"):
        P(f"  512^3 {prec} pcg mg, ms per launch (launches): "
          + ", ".join(f"{k} {ms:.4f} ({c})" for k, (c, ms) in level_kernels(512, prec).items()))
    n = 128
    with tempfile.TemporaryDirectory(prefix="cz_mgd_") as out:
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "rank", str(r), "2", out, str(n)], env=rank_env(r),
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
        logs = [p.communicate(timeout=300)[0] for p in procs]
        if any(p.returncode for p in procs):
            print("\n".join(logs))
            sys.exit(1)
        recs = [json.load(open(os.path.join(out, f"rank_{r}.json"))) for r in range(2)]
    P("")
    P(f"two RCCL ranks SHARING ONE GPU (division 2x1x1, {n}^3 FP64; socket transport over loopback; not a scaling measurement)")
    for rec in recs:
        i = rec["info"]
        P(f"  rank {rec['rank']}: V-cycle incl. the host copies of r and z {rec['t_cycle_s'] * 1e3:8.2f} ms (one field copy alone "
          f"{rec['t_d2h_s'] * 1e3:.2f} ms); levels {i['mg_levels']}, gather level {i['mg_gather_level']}, exchanges per V-cycle "
          f"{i['mg_exchanges']}; solve {rec['itr']} iterations, {rec['solve_s'] / max(rec['itr'], 1) * 1e3:.3f} ms/iteration")
    G, rows = bytes_model(n, (2, 1, 1), 0)
    P(f"  bytes rank 0 sends per exchange (model, FP64), levels 0 .. {G - 1} distributed, level {G} on: all-gathered")
    for lev, c, face, full in rows:
        P(f"    level {lev}: owned {c[0]}x{c[1]}x{c[2]}, face exchange {face} B, face + edge + corner exchange {full} B")
    print("\n".join(lines))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "rank":
        rank_main(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5]))
    else:
        main()
