"""Line-fetch model of jac3_k (three Jacobi sweeps per pass) at n^3: bytes per launch by workgroup order and chunk length.
    python3 tools/line_model.py [n] [kwin] [tj ...]
Rule: a 128-byte line is fetched once per XCD per (chunk, plane) if any workgroup of that chunk running in the same round on that XCD reads
it; nothing is reused across chunks, rounds or XCDs.  Orders: 'win' = window-major segment ids cut into eight runs (CZHIP_T2_MAP=2 and
before), 'row' = every window of a band of row segments on one XCD (pair_xcd_map with nwin > 1, the default).  A model, not a measurement:
profiles/r10/pass_planner.txt sets it against the FETCH_SIZE / WRITE_SIZE counters."""
import math
import sys

import numpy as np

V, LINE, TB, HALO_ROWS, HV, SLOTS = 4, 32, 1024, 4, 1, 32  # FP32 vectors, floats per line, threads, halo rows (+-2), halo vectors, CUs per XCD


def geom(n, kwin):
    nkp = nip = n + 4
    rf = math.ceil(nkp / V)
    nwin = math.ceil(rf / kwin)
    kt = math.ceil(rf / nwin)
    r = kt + 2 * HV
    s = TB - HALO_ROWS * r
    f0, fend = 2 * r, (n + 2) * r  # rows ii0 = 2 .. ii1 = n + 1
    return dict(n=n, nkp=nkp, nip=nip, R=r, KT=kt, nwin=nwin, S=s, F0=f0, Fend=fend, nsegw=math.ceil((fend - f0) / s))


def lines(g, w, s, rows_extra):
    """the lines a workgroup of window w, row segment s reads on one plane of an operand it needs rows_extra rows beyond its segment of"""
    r = g["R"]
    fb = g["F0"] + s * g["S"]
    f = np.arange(fb - rows_extra * r, min(fb + g["S"], g["Fend"]) + rows_extra * r)
    f = np.clip(f, 0, r * g["nip"] - 1)
    el = (f // r) * g["nkp"] + w * g["KT"] * V - HV * V + (f % r) * V
    return np.unique(np.maximum(el, 0) // LINE)


def launch_bytes(g, order, tj):
    n, nwin, nsegw = g["n"], g["nwin"], g["nsegw"]
    nseg, nch = nwin * nsegw, math.ceil(n / tj)
    ids = [(i // nsegw, i % nsegw) for i in range(nseg)] if order == "win" else [(i % nwin, i // nwin) for i in range(nseg)]
    per, tot = math.ceil(nseg / 8), 0
    for x in range(8):
        band = ids[x * per:(x + 1) * per]
        u = {ws: lines(g, *ws, 3) for ws in band}  # u: segment +- 3 rows, b: +- 2
        b = {ws: lines(g, *ws, 2) for ws in band}
        items = [(c, ws) for c in range(nch) for ws in band]
        for r0 in range(0, len(items), SLOTS):
            rnd = items[r0:r0 + SLOTS]
            for c in sorted(set(c for c, _ in rnd)):
                mem = [ws for cc, ws in rnd if cc == c]
                nu = len(np.unique(np.concatenate([u[m] for m in mem])))
                nb = len(np.unique(np.concatenate([b[m] for m in mem])))
                planes = min(tj, n - c * tj)
                tot += nu * (planes + 6) + nb * (planes + 4)  # +6 / +4: the halo planes a chunk re-reads
    reads, writes = tot * LINE * 4, n ** 3 * 4
    return reads + writes, math.ceil(nseg * nch / 8 / SLOTS)


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    kwin = int(sys.argv[2]) if len(sys.argv) > 2 else 26
    tjs = [int(a) for a in sys.argv[3:]] or [32, 171]
    g = geom(n, kwin)
    fused = 3 * n ** 3 * 4  # one fused pass: read u and b, write w
    print(f"{n}^3 FP32, windows of {kwin} vectors: R = {g['R']}, S = {g['S']}, {g['nwin']} windows x {g['nsegw']} row segments")
    for tj in tjs:
        for order in ("win", "row"):
            by, rounds = launch_bytes(g, order, tj)
            print(f"  order {order}  TJ {tj:4d}  rounds {rounds}:  {by / 1e9:.3f} GB per launch = {by / fused:.2f} x the fused minimum")
