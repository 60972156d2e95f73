"""CPU tests: the oracle (C restatement) against the golden fixtures generated from the reference's
own Fortran (tests/golden/make_golden.py), and -- stored, and when oracle/_ref is present also directly -- against
the reference library on fresh random inputs.  All bit-exact (single thread, no contraction)."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import cz_oracle as O

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = json.load(open(os.path.join(GOLDEN, "solver_cases.json")))


def _beq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_kernels_match_golden(prec):
    g = np.load(os.path.join(GOLDEN, f"kernels_{prec}.npz"))
    k = O.Kernels("oracle", prec)
    sz, idx, cf, omg = list(g["sz"]), list(g["idx"]), g["cf"], float(g["omg"])
    p, b, q, x, y, z = (g[n] for n in ("in_p", "in_b", "in_q", "in_x", "in_y", "in_z"))

    pj, wk = p.copy(), np.zeros_like(p)
    res = k.jacobi(pj, sz, idx, cf, omg, b, wk, res=0.25)
    assert _beq(pj, g["jacobi_p"]) and _beq(wk, g["jacobi_wk2"])
    assert res == float(g["jacobi_res"]) and k.last_flop == float(g["jacobi_flop"])

    for ofst in (0, 1):
        ps, r = p.copy(), 0.0
        for color in (0, 1):
            r = k.psor2sma_core(ps, sz, idx, cf, ofst, color, omg, b, res=r)
            assert _beq(ps, g[f"rb{ofst}_p_c{color}"])
            assert r == float(g[f"rb{ofst}_res_c{color}"])

    ap = np.zeros_like(p)
    k.blas_calc_ax(ap, p, sz, idx, cf)
    assert _beq(ap, g["calc_ax"])
    rk = np.zeros_like(p)
    k.blas_calc_rk(rk, p, b, sz, idx, cf)
    assert _beq(rk, g["calc_rk"])
    assert k.blas_dot1(p, sz, idx) == g["dot1"]
    assert k.blas_dot2(p, q, sz, idx) == g["dot2"]
    zt = z.copy()
    k.blas_triad(zt, x, y, -0.37, sz, idx)
    assert _beq(zt, g["triad"])
    pb = p.copy()
    k.blas_bicg_1(pb, x, q, 0.61, -1.3, sz, idx)
    assert _beq(pb, g["bicg_1"])
    zb = z.copy()
    k.blas_bicg_2(zb, x, y, 0.45, -0.77, sz, idx)
    assert _beq(zb, g["bicg_2"])
    c = p.copy()
    k.blas_clear(c, sz)
    assert _beq(c, g["clear"])
    d = np.zeros_like(p)
    k.blas_copy(d, p, sz)
    assert _beq(d, g["copy"])
    for tag, nid, org in (("all", [-1] * 6, [0.0, 0.0, 0.0]), ("mix", [3, -1, -1, 5, -1, 2], [0.25, 0.5, 0.0])):
        pc = p.copy()
        k.bc_k(sz, pc, 1.0 / (sz[2] - 1), org, nid)
        assert _beq(pc, g[f"bc_{tag}"])
    e = np.zeros_like(p)
    k.exact_t(sz, e, 1.0 / (sz[2] - 1), [0.0, 0.0, 0.0])
    assert _beq(e, g["exact"])

    # MAF flavour on the stretched grid
    xc, yc, zc = g["maf_x"], g["maf_y"], g["maf_z"]
    pv = g["maf_pvt_in"].copy()
    k.search_pivot(pv, sz, idx, xc, yc, zc)
    assert _beq(pv, g["maf_pvt"])
    pm, wm = p.copy(), np.zeros_like(p)
    res = k.jacobi_maf(pm, sz, idx, xc, yc, zc, omg, b, wm, res=0.5)
    assert _beq(pm, g["maf_jacobi_p"]) and _beq(wm, g["maf_jacobi_wk2"])
    assert res == float(g["maf_jacobi_res"]) and k.last_flop == float(g["maf_jacobi_flop"])
    for ofst in (0, 1):
        ps, r = p.copy(), 0.0
        for color in (0, 1):
            r = k.psor2sma_core_maf(ps, sz, idx, xc, yc, zc, ofst, color, omg, b, res=r)
            assert _beq(ps, g[f"maf_rb{ofst}_p_c{color}"]) and r == float(g[f"maf_rb{ofst}_res_c{color}"])
    a = g["maf_ax_in"].copy()
    k.calc_ax_maf(a, p, sz, idx, xc, yc, zc, pv)
    assert _beq(a, g["maf_ax"])
    a = g["maf_rk_in"].copy()
    k.calc_rk_maf(a, p, b, sz, idx, xc, yc, zc, pv)
    assert _beq(a, g["maf_rk"])

    # lexicographic point SOR, one thread
    pp = g["in_p"].copy()
    assert k.psor(pp, sz, idx, cf, omg, b, res=0.125) == float(g["psor_res"]) and _beq(pp, g["psor_p"])
    assert k.last_flop == float(g["psor_flop"])
    pp = g["in_p"].copy()
    assert k.psor_maf(pp, sz, idx, xc, yc, zc, omg, b, res=0.125) == float(g["maf_psor_res"]) and _beq(pp, g["maf_psor_p"])

    # line SOR by PCR (fixtures from the reference's serial build)
    for (ni, nj, nk) in ((9, 8, 13), (12, 10, 37), (6, 7, 64)):
        szp, idp, tag = [ni, nj, nk], [2, ni - 1, 2, nj - 1, 2, nk - 1], f"pcr_{ni}x{nj}x{nk}"
        xx, mk = g[tag + "_x_in"].copy(), g[tag + "_x_in"].copy()
        k.imask_k(mk, szp, idp)
        assert _beq(mk, g[tag + "_msk"])
        r = 0.0
        for color in (0, 1):
            r = k.pcr_rb(szp, idp, O.get_num_stage(idp[5] - idp[4] + 1), 0, color, xx, mk, g[tag + "_rhs"], 1.1, res=r)
            assert _beq(xx, g[tag + f"_x_c{color}"]) and r == float(g[tag + f"_res_c{color}"])
        assert k.last_flop == float(g[tag + "_flop"])


def test_wide_accumulators_consistent():
    """the *_w entry points return the same REAL result plus a double accumulation of the same terms."""
    g = np.load(os.path.join(GOLDEN, "kernels_f32.npz"))
    k = O.Kernels("oracle", "f32")
    sz, idx = list(g["sz"]), list(g["idx"])
    p, b = g["in_p"], g["in_b"]
    w = np.zeros(1)
    pj, wk = p.copy(), np.zeros_like(p)
    res = k.jacobi(pj, sz, idx, g["cf"], float(g["omg"]), b, wk, res=0.25, wide=w)
    assert res == float(g["jacobi_res"])
    dp = (pj - p).astype(np.float32)[2:-2, 2:-2, 2:-2]
    # dp*dp rounded to float then summed in double == the wide accumulator up to order of summation
    assert abs(w[0] - float(np.sum((dp * dp).astype(np.float64)))) < 5e-5 * w[0]
    w[:] = 0
    assert k.blas_dot1(p, sz, idx, wide=w) == g["dot1"]
    inner = p[3:-3, 3:-3, 3:-3]
    assert abs(w[0] - float(np.sum((inner * inner).astype(np.float64)))) < 1e-12 * w[0]


# 128^3 BiCGSTAB cases cost ~10 s each on one core: keep two, skip nothing silently
SMALL = [c for c in CASES if max(c["gsz"]) <= 64 or c["tag"] in ("jacobi_128x128x128_f32", "pbicgstab_sor2sma_128x128x128_f64")]


@pytest.mark.parametrize("case", SMALL, ids=[c["tag"] for c in SMALL])
def test_solver_histories_match_golden(case):
    r = O.run(case["gsz"], case["solver"], case["itr_max"], case["coef"], case["precond"], kind="oracle",
              prec=case["prec"], with_error=True)
    assert r.itr == case["iter"]
    assert r.res == case["res"]
    if case["cli"]:  # what the reference CLI printed
        assert r.itr == case["cli"][0] and "%e" % r.res == case["cli"][1]
    assert r.history_text() == open(os.path.join(GOLDEN, f"hist_{case['tag']}.txt")).read()
    assert hashlib.sha256(r.P.tobytes()).hexdigest() == case["sha256_P"]
    if "field" in case:
        assert _beq(r.P, np.load(os.path.join(GOLDEN, case["field"])))
    assert r.errmax == case["errmax"] and list(r.errloc) == case["errloc"]


def random_box_record(k):
    """fresh random inputs, anisotropic boxes, both colours/offsets, through one back-end: every scalar it returns (exact, float.hex) and the
    sha256 of every array it writes, in call order.  Two back-ends agree bit for bit iff their records are equal."""
    rec = []

    def put(*vals):
        for v in vals:
            rec.append(hashlib.sha256(v.tobytes()).hexdigest() + f" {v.dtype} {v.shape}" if isinstance(v, np.ndarray) else float(v).hex())

    rng = np.random.default_rng(7)
    for (ni, nj, nk) in ((5, 4, 6), (9, 12, 7), (16, 8, 33)):
        sz = [ni, nj, nk]
        shape = (nj + 4, ni + 4, nk + 4)
        idx = [2, ni - 1, 2, nj - 1, 2, nk - 1] if ni > 5 else [1, ni, 1, nj, 1, nk]  # also the interior-rank range
        cf = rng.uniform(0.5, 1.5, 7).astype(k.real)
        cf[6] = 6.2
        p = rng.uniform(-1, 1, shape).astype(k.real)
        b = rng.uniform(-1, 1, shape).astype(k.real)
        q = rng.uniform(-1, 1, shape).astype(k.real)
        a, w = p.copy(), np.zeros_like(p)
        put(k.jacobi(a, sz, idx, cf, 0.9, b, w, res=1.5), a, w)
        for ofst in (0, 1):
            a, r = p.copy(), 0.0
            for color in (0, 1):
                r = k.psor2sma_core(a, sz, idx, cf, ofst, color, 1.3, b, res=r)
                put(r, a)
        a = np.zeros_like(p)
        k.blas_calc_ax(a, p, sz, idx, cf)
        put(a)
        k.blas_calc_rk(a, p, b, sz, idx, cf)
        put(a)
        put(k.blas_dot1(p, sz, idx), k.blas_dot2(p, q, sz, idx))
        a = q.copy()
        k.blas_bicg_1(a, p, b, 0.3, 0.7, sz, idx)
        put(a)
        k.blas_bicg_2(a, p, b, 0.3, 0.7, sz, idx)
        put(a)
        k.blas_triad(a, p, b, -0.3, sz, idx)
        put(a)
        a = p.copy()
        for nid in ([-1] * 6, [0, 1, -1, -1, 2, -1]):
            k.bc_k(sz, a, 0.125, [0.1, 0.2, 0.3], nid)
            put(a)
    return rec


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_oracle_vs_reference_random_boxes(prec):
    """fresh random inputs, anisotropic boxes, both colours/offsets: restatement == reference, bit for bit -- against the reference's record
    stored in tests/golden/ref_random_boxes.json (tests/golden/make_golden.py), and against the reference library itself where oracle/_ref
    is built."""
    got = random_box_record(O.Kernels("oracle", prec))
    want = json.load(open(os.path.join(GOLDEN, "ref_random_boxes.json")))[prec]
    assert got == want
    if O.have("ref", prec):
        assert got == random_box_record(O.Kernels("ref", prec))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_sph_writer_restatement_matches_the_reference_file(prec):
    """.sph field file (cz_utility.f90:17-47, written by the reference built with -D_aurora_=1): the restatement used to check
    the GPU driver's p_00000.sph / e_00000.sph produces the reference's bytes."""
    g = np.load(os.path.join(GOLDEN, f"kernels_{prec}.npz"))
    R = np.float32 if prec == "f32" else np.float64
    want = open(os.path.join(GOLDEN, f"sph_small_{prec}.sph"), "rb").read()
    got = O.sph_bytes([5, 4, 6], g["sph_in"], R(0.25), np.array([0.5, 0.25, 0.125], dtype=R))
    assert got == want


def _bicg_parity():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bicg_parity
    return bicg_parity


@pytest.mark.parametrize("case", [c for c in _bicg_parity().CASES + _bicg_parity().DECOMP_CASES], ids=lambda c: c["id"])
def test_bicgstab_parity_premise(case):
    """The premise of tests/test_gpu_bicgstab_parity.py on the oracle alone: FP32 -- no dot product of the K iterations lies within its
    summation bound of a float rounding boundary, and the runs with every dot at either edge of the bound are bit-identical to the unperturbed
    one; FP64 -- the envelope of those runs stays below 1e-8 relative at every compared iteration count.  A failure here means: choose
    another case, not: the GPU is wrong."""
    BP = _bicg_parity()
    if case["prec"] == "f32":
        r = BP.premise_f32(case)
    else:
        for k in BP.ks(case):
            r, _, _ = BP.envelope_f64(case, k + 1)
    assert len(r.history) >= 3, "too short to say much about the recurrence"


def test_exact_dot_mode_logs_every_dot_and_leaves_the_wide_path_alone():
    """dots="exact": five dots per iteration, each the correctly rounded sum of the REAL products, within its bound of the wide (double,
    loop-order) sum; the wide mode's result does not depend on the new mode existing."""
    args = ((20, 18, 22), "pbicgstab", 4, 0.8, "jacobi")
    for prec in ("f32", "f64"):
        e = O.run(*args, prec=prec, dots="exact")
        w = O.run(*args, prec=prec, wide=True)
        assert [x[1] for x in e.dot_log] == ["rho", "q.r0", "t.s", "t.t", "r.r"] * len(e.history)
        assert all(B > 0 and n == 18 * 16 * 20 for (_, _, _, B, n) in e.dot_log)
        assert e.itr == w.itr
        assert np.allclose([r for _, r in e.history], [r for _, r in w.history], rtol=1e-6 if prec == "f32" else 1e-12, atol=0)
        w2 = O.run(*args, prec=prec, wide=True)
        assert w2.P.tobytes() == w.P.tobytes() and w2.history == w.history and w.dot_log == []
