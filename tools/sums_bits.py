"""The raw bits of every sum the kernels hand back through the last-workgroup hand-off (cz_k_sums.h), for an A/B of two builds:
    python3 tools/sums_bits.py LIBDIR f32|f64 > out.txt      (LIBDIR holds libczhip_f32.so / libczhip_f64.so; one process per run)
Two builds compute the same sums in the same order exactly when their outputs are byte-identical (profiles/r32/sums_bits.txt).  The suite
cannot see a reordered sum: its comparisons are made immune to the order on purpose.

Every case goes through an existing C entry or the driver.  The fields hold signed values whose magnitudes spread over 20 binades, so the
products and squares that are summed spread over 40 and the sum depends on the order of its additions.  The script checks that premise
itself: the numpy sum of a case's terms (the per-point products of a dot; the squared change of the field for a sweep; the squared
residual, the squared divergence; b^2 for a whole solve), taken forward and taken in reversed order, must differ in bits.  A case whose
data fail that (a few large terms decide such a sum about every other time) is replaced: it runs again with the next seed, up to SEEDS
of them, and its line names the seed it passed with.  A case that never passes is printed as PREMISE FAILS and the status is 1.

Boxes (ni x nj x nk, odd extents: every edge mask is partial), chosen off the launchers of cz_kernels.hip, cz_h_launch.h and cz_h_linesor.h:
    one    13 x 3 x 9, ONE inner plane j: dot_k and its kin launch (1, min(planes, 4096)) workgroups, stencil_k (tuning 256 threads, 1 vector,
           1 plane per chunk) segments x chunks = 1 x 1: a single workgroup
    few    13 x 11 x 9, all inner planes: 9 workgroups in those kernels (between 2 and the 256 threads of a workgroup)
    many   13 x 261 x 9: 259 planes -> 259 workgroups of 256 threads (stencil_k pads the chunks to 264): a finishing thread adds two partials
    tall   13 x 2601 x 9: psor_col_k gathers one partial per 8 x 8 column, 2 x 325 = 650 of them against its 384 or 640 threads; the fused
           passes with two planes per chunk launch 1 300 chunks, more workgroups than their 1 024 threads.  pcr_lex_wg_k is also asked for
           one group and one row per thread (a strip per row); the launches traced (profiles/r32/sums_bits.txt) had 33 strips against 512 threads
           at most all the same: its finishing threads add one partial at most here
The line solvers, psor_ and the driver's passes size their grids by the device as well (columns or strips against CUs x workgroups per
CU); they run on the first three boxes, the driver's cases on few and many: a brick has three planes at least, and resid_row_k, div_row_k,
div_any_k and ax_coef_k launch one row of workgroups per plane, so no box gives them a single workgroup.  The `more` hook of pass_epilogue
(the shell sums of a split pass) exists in decomposed runs only and is not reached from here.  The workgroup counts as launched:
rocprofv3 --kernel-trace of one run, in the record.
"""
import ctypes as C
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cubez_amd.lib as czlib  # noqa: E402


def hexd(v):
    return struct.pack(">d", float(v)).hex()


def hexr(v, real):
    return np.asarray(v, dtype=real).tobytes()[::-1].hex()


SEEDS = 24


def premise(terms):
    t = np.asarray(terms, dtype=np.float64).ravel()
    t = t[t != 0.0]
    return t.size > 1 and hexd(np.add.reduce(t)) != hexd(np.add.reduce(t[::-1]))


def wide(rng, shape, real):
    """signed, magnitudes 2^-10 .. 2^10"""
    return (rng.choice([-1.0, 1.0], shape) * np.exp2(rng.uniform(-10.0, 10.0, shape))).astype(real)


def inner(a, idx):
    i0, i1, j0, j1, k0, k1 = idx
    return a[j0 + 1:j1 + 2, i0 + 1:i1 + 2, k0 + 1:k1 + 2]  # 1-based index + guide 2, 0-based array


def run_cases(box, make_data, cases):
    """cases: [(label, fn(data) -> (hex values, terms))]; every case with the first seed whose terms pass the premise"""
    done, failed = {}, 0
    for seed in range(SEEDS):
        todo = [(label, fn) for label, fn in cases if label not in done]
        if not todo:
            break
        data = make_data(seed)
        for label, fn in todo:
            values, terms = fn(data)
            if premise(terms):
                done[label] = f"{label:34s} {box:5s} seed {seed:2d}  {' '.join(values)}"
    for label, _ in cases:
        print(done.get(label, f"{label:34s} {box:5s} PREMISE FAILS with every seed"), flush=True)
        failed += label not in done
    return failed


def kernels(prec, box, sz, idx, only=None):
    h = czlib.CzHip(prec)
    real = h.real
    shape = (sz[1] + 4, sz[0] + 4, sz[2] + 4)
    assert h.set_tuning(256, 1, 1, 0)
    cf = [1, 1, 1, 1, 1, 1, 6]
    (_, szp), (_, idxp) = h._i(sz), h._i(idx)
    cgu = h.lib.czhip_cg_update_async
    cgu.argtypes = [C.c_void_p] * 5 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    cgu.restype = None
    sc = h.dbuf(5, real).put(np.array([0.37, -0.37, 0, 0, 0.0123], dtype=real))
    m = h.dbuf(1, real).put(np.array([0.5], dtype=real))
    dots = h.dbuf(2, np.float64)
    mask = np.zeros(shape, dtype=real)
    msk = h.alloc(sz, mask)
    h.imask_k(msk, sz, idx)
    pn = 1
    while (1 << pn) <= idx[5] - idx[4] + 1:
        pn += 1

    def make_data(seed):
        rng = np.random.default_rng(1000 + seed)
        d = {n: wide(rng, shape, real) for n in "PQRX"}
        d["xyz"] = [np.cumsum(rng.uniform(0.5, 1.5, n + 4)).astype(real) for n in sz]
        return d

    def sq(new, old):
        d = inner(new, idx).astype(np.float64) - inner(old, idx)
        return d * d

    def dot1(d):
        dP = h.alloc(sz, d["P"])
        v = hexr(h.blas_dot1(dP, sz, idx), real)
        dP.free()
        return [v], inner(d["P"], idx) * inner(d["P"], idx)

    def dot2(d):
        dP, dQ = h.alloc(sz, d["P"]), h.alloc(sz, d["Q"])
        v = hexr(h.blas_dot2(dP, dQ, sz, idx), real)
        dP.free(), dQ.free()
        return [v], inner(d["P"], idx) * inner(d["Q"], idx)

    def cg_update(closed):
        def fn(d):
            dx, dr, dP, dQ = (h.alloc(sz, d[n]) for n in "XRPQ")
            if closed:
                h.cg_update_closed(dx, dr, dP, dQ, sc, sz, idx, dots)
            else:
                cgu(dx.ptr, dr.ptr, dP.ptr, dQ.ptr, sc.ptr, szp, idxp, czlib.GUIDE, dots.ptr)
            out = dots.get()
            rn = inner(dr.get(), idx).astype(np.float64)
            for a in (dx, dr, dP, dQ):
                a.free()
            return [hexd(v) for v in out[:2 if closed else 1]], rn * rn
        return fn

    def shift(store):
        def fn(d):
            da = h.alloc(sz, d["P"])
            assert h.shift_sums(da, m if store else None, sz, idx, dots)
            an = inner(da.get(), idx).astype(np.float64)
            da.free()
            return [hexd(v) for v in dots.get()], an * an
        return fn

    def sweep(call, src="P"):  # an in-place (or, Jacobi, out-of-place) sweep: the terms are the squared change of the field
        def fn(d):
            dx, db = h.alloc(sz, d[src]), h.alloc(sz, d["Q"])
            res, new = call(dx, db, d)
            new = dx.get() if new is None else new
            dx.free(), db.free()
            return [hexd(res)], sq(new, d[src])
        return fn

    def jacobi(dx, db, d):
        dw = h.alloc(sz, d["P"])
        res = h.jacobi(dx, sz, idx, cf, 0.8, db, dw)
        new = dw.get()
        dw.free()
        return res, new

    def rb(dx, db, d):  # both colours: the second launch accumulates onto the first one's sum
        res = h.psor2sma_core(dx, sz, idx, cf, 0, 0, 1.1, db)
        return h.psor2sma_core(dx, sz, idx, cf, 0, 1, 1.1, db, res=res), None

    def pcr_rb(form):
        def call(dx, db, d):
            h.lib.czhip_set_pcr_mode(form, 0)
            res = h.pcr_rb(sz, idx, pn, 0, 0, dx, msk, db, 1.1)
            res = h.pcr_rb(sz, idx, pn, 0, 1, dx, msk, db, 1.1, res=res)
            h.lib.czhip_set_pcr_mode(2, 0)
            return res, None
        return call

    q_default = czlib.tuning_in_force(h.lib)["pcr_q"]

    def pcr_lex(one, maf, narrow=0):
        def call(dx, db, d):
            h.lib.czhip_set_pcr_lex(one, narrow, narrow if narrow else -1)
            res = h.pcr_maf("pcr_maf", sz, idx, pn, 0, dx, msk, db, *d["xyz"], 1.1) if maf else h.pcr(sz, idx, pn, dx, msk, db, 1.1)
            h.lib.czhip_set_pcr_lex(1, 0, q_default)
            return res, None
        return call

    def pcr_rb_maf(dx, db, d):
        res = h.pcr_maf("pcr_rb_maf", sz, idx, pn, 0, dx, msk, db, *d["xyz"], 1.1)
        return h.pcr_maf("pcr_rb_maf", sz, idx, pn, 1, dx, msk, db, *d["xyz"], 1.1, res=res), None

    cases = [("blas_dot1_", dot1), ("blas_dot2_", dot2), ("czhip_cg_update_async", cg_update(False)),
             ("czhip_cg_update_closed_async", cg_update(True)), ("czhip_shift_sums_async shift", shift(True)),
             ("czhip_shift_sums_async read", shift(False)), ("jacobi_", sweep(jacobi)), ("psor2sma_core_ colours 0, 1", sweep(rb)),
             ("psor_", sweep(lambda dx, db, d: (h.psor(dx, sz, idx, cf, 1.1, db), None)))]
    cases += [(f"pcr_rb_ form {f} colours 0, 1", sweep(pcr_rb(f), "X")) for f in (0, 1, 2)]  # pcr_rb_k, pcr_rb2_k, pcr_line_reg_k
    cases += [(f"pcr_{'maf_' if maf else ''} one_launch {one}", sweep(pcr_lex(one, maf), "X")) for one in (1, 0) for maf in (0, 1)]
    cases += [("pcr_rb_maf_ colours 0, 1", sweep(pcr_rb_maf, "X"))]  # pcr_line_reg_maf_k
    # one group of threads and one row per thread: a strip is a row, nj strips gathered by 64 threads
    cases += [("pcr_ one_launch 1, 1 group, 1 row", sweep(pcr_lex(1, 0, 1), "X"))]
    if only is not None:
        cases = [c for c in cases if c[0] in only]
    return run_cases(box, make_data, cases)


def driver(prec, box, size, planes=0):
    from cubez_amd.driver import CZ
    real = np.float32 if prec == "f32" else np.float64
    ni, nj, nk = size

    def make_data(seed):
        rng = np.random.default_rng(2000 + seed)
        d = {n: wide(rng, (ni, nj, nk), real) for n in ("b", "p0", "u", "v", "w")}
        d["beta"] = [np.exp2(rng.uniform(-3.0, 3.0, (ni, nj, nk))).astype(real) for _ in range(3)]
        return d

    def handle(d, args, deep=False):
        cz = CZ(prec)
        if deep:  # the fused passes also on small grids (pass_epilogue: jacobi2p_k, jac3_k, jac4_k, rb4_k)
            for setter in (cz.lib.czhip_set_jac3, cz.lib.czhip_set_jac4, cz.lib.czhip_set_rb4):
                setter(2, -1, planes if planes else -1)
            if planes:  # the two-stage pass as well
                assert cz.lib.czhip_set_tuning2(0, 0, planes, -1) == 0
        assert cz.setup([str(v) for v in size] + args) == 1
        cz.set_rhs(d["b"])
        cz.set_field(d["p0"])
        cz.set_eps(1.0e-300)
        return cz

    def bb(d):
        return d["b"][1:-1, 1:-1, 1:-1].astype(np.float64) ** 2

    # the solvers' own sums: the residual history is made of them (BiCGSTAB: triad_dots_k, stencil_k's ax_dots; PCG: cg_update_k, MODE_DIRAX;
    # the stationary solvers: stencil_k and, deep, the fused passes)
    def solve(args, deep, residual):
        def fn(d):
            cz = handle(d, args, deep)
            cz.solve()
            values, terms = [hexd(v) for v in cz.history()], bb(d)
            if residual:  # resid_row_k on the field the solve left
                out, ss = cz.get_residual(dtype=real)
                values, terms = [hexd(ss)], out.astype(np.float64) ** 2
            cz.close()
            return values, terms
        return fn

    def div(transposed):  # div_row_k | div_any_k
        def fn(d):
            u, v, w = ((np.asfortranarray(d[n]) if transposed else d[n]) for n in "uvw")
            dd = ((u[1:-1, 1:-1, 1:-1] - u[:-2, 1:-1, 1:-1]) + (v[1:-1, 1:-1, 1:-1] - v[1:-1, :-2, 1:-1])) + (w[1:-1, 1:-1, 1:-1] - w[1:-1, 1:-1, :-2])
            cz = handle(d, ["pcg", "4", "0.8", "jacobi"])
            ss = cz.set_rhs_div(u, v, w)
            cz.close()
            return [hexd(ss)], dd.astype(np.float64) ** 2
        return fn

    def coef(solve_too):  # ax_coef_k: MODE 1 in cz_get_residual, MODE 0 in the solve
        def fn(d):
            cz = handle(d, ["pcg", "4", "0.8", "jacobi"])
            cz.set_face_coef(*d["beta"])
            out, ss = cz.get_residual(dtype=real)
            values, terms = [hexd(ss)], out.astype(np.float64) ** 2
            if solve_too:
                cz.solve()
                values, terms = [hexd(v) for v in cz.history()], bb(d)
            cz.close()
            return values, terms
        return fn

    def closed(d):  # shift_sums_k and cg_update_k<V, true> inside a solve
        cz = handle(d, ["pcg", "5", "0.8", "jacobi"])
        cz.set_closed_box(True)
        cz.set_rhs(d["b"])
        cz.solve()
        values = [hexd(v) for v in cz.history()] + [hexd(cz.closed_mean(q)) for q in (0, 1, 2)]
        cz.close()
        return values, bb(d)

    cases = []
    for args, deep in ((["pbicgstab", "6", "0.8", "jacobi"], False), (["pcg", "6", "0.8", "jacobi"], False), (["pcg", "6", "1.2", "mgrb"], False),
                       (["jacobi", "12", "0.8"], False), (["jacobi", "12", "0.8"], True), (["sor2sma", "8", "1.1"], True)):
        label = " ".join(args[:1] + args[3:]) + (" deep" if deep else "")
        cases += [("cz_solve " + label, solve(args, deep, False))]
        if "mgrb" not in args:  # (six V-cycles leave a residual of a few units in the last place on these boxes: its squares prove nothing)
            cases += [("cz_get_residual after " + label, solve(args, deep, True))]
    if planes:  # the tall box: the fused passes alone, `planes` planes per chunk, so that a launch has more workgroups than 1024 threads
        return run_cases(box, make_data, [c for c in cases if " deep" in c[0] and c[0].startswith("cz_solve")])
    cases += [("cz_set_rhs_div rows", div(False)), ("cz_set_rhs_div any strides", div(True)), ("cz_set_face_coef, cz_get_residual", coef(False)),
              ("cz_set_face_coef, cz_solve pcg", coef(True)), ("cz_solve pcg closed box", closed)]
    return run_cases(box, make_data, cases)


def main():
    libdir, prec = os.path.abspath(sys.argv[1]), sys.argv[2]
    czlib.lib_path = lambda p: os.path.join(libdir, f"libczhip_{p}.so")
    print(f"# sums_bits {prec}", flush=True)
    failed = 0
    for box, sz, idx in (("one", [13, 3, 9], [2, 12, 2, 2, 2, 8]), ("few", [13, 11, 9], [2, 12, 2, 10, 2, 8]),
                         ("many", [13, 261, 9], [2, 12, 2, 260, 2, 8])):
        failed += kernels(prec, box, sz, idx)
    failed += kernels(prec, "tall", [13, 2601, 9], [2, 12, 2, 2600, 2, 8], only=("psor_", "pcr_ one_launch 1, 1 group, 1 row"))
    for box, size in (("few", (13, 11, 9)), ("many", (13, 261, 9))):
        failed += driver(prec, box, size)
    failed += driver(prec, "tall", (13, 2601, 9), planes=2)
    print(f"# PREMISE FAILS in {failed} cases" if failed else "# every case's premise holds")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
