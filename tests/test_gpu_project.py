"""The projection step on a staggered velocity on the GPU (-m gpu), every result against the numpy restatement of
tests/project_parity.py: cz_set_rhs_div and cz_sub_grad byte for byte in every layout, from device tensors and from numpy arrays, in both
kernel forms; CZ.project end to end in the six states under the bars the restatement gives; the stream hand-over; the refusals."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_parity as CB  # noqa: E402
import periodic_parity as P  # noqa: E402
import problem_parity as PP  # noqa: E402
import project_parity as J  # noqa: E402
import test_gpu_neumann as TN  # noqa: E402
from test_gpu_periodic import _handle  # noqa: E402
from test_gpu_problem import _real, _torch  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = [(9, 7, 12), (33, 47, 61), (3, 40, 40), (40, 40, 1100)]  # the last: long rows with vector body, head and tail
SHAPE_IDS = ["x".join(map(str, g)) for g in SHAPES]
LAYOUTS = ("c_order", "fortran", "interleaved", "k_strided", "slice")
ROW_FORM = {"c_order": 1, "fortran": 3, "interleaved": 3, "k_strided": 3, "slice": 1}
OUTSIDE, KEEP = 777.0, -999.25  # sentinels: elements of a base array outside the brick; elements of the brick that sub_grad must not write
SCALE = 1.7  # (not a power of two: the product rounds)
SOLVER = ["pcg", 50, 1.2, "mgrb"]


def _arrays(layout, gsz, R):
    """(bases, views): numpy base arrays full of OUTSIDE and the function that gives the three bricks [i, j, k] of equal strides inside a
    list of bases (numpy arrays or torch tensors)"""
    ni, nj, nk = gsz
    tr = lambda b: b.transpose(2, 1, 0) if isinstance(b, np.ndarray) else b.permute(2, 1, 0)  # noqa: E731
    if layout == "interleaved":
        return [np.full((ni, nj, nk, 3), OUTSIDE, dtype=R)], lambda bs: [bs[0][..., c] for c in range(3)]
    shape, view = {"c_order": ((ni, nj, nk), lambda b: b), "fortran": ((nk, nj, ni), tr), "k_strided": ((ni, nj, 2 * nk + 1), lambda b: b[:, :, 1::2]),
                   "slice": ((ni + 2, nj + 3, nk + 5), lambda b: b[1:1 + ni, 2:2 + nj, 3:3 + nk])}[layout]
    return [np.full(shape, OUTSIDE, dtype=R) for _ in range(3)], lambda bs: [view(b) for b in bs]


def _placed(layout, gsz, R, vel):
    bases, views = _arrays(layout, gsz, R)
    for dst, src in zip(views(bases), vel):
        dst[...] = src
    return bases, views


def _on(torch, bases):
    return [torch.from_numpy(b).cuda() for b in bases] if torch is not None else bases


def _back(bases):
    return [b if isinstance(b, np.ndarray) else b.cpu().numpy() for b in bases]


def _rhs(cz, gsz, R):
    """the right-hand side in the handle at the inner cells, with no new getter: the residual of a zero field is b"""
    cz.set_field(np.zeros(gsz, dtype=R))
    return cz.get_residual(dtype=R)[0]


def _check_div(cz, prec, gsz, name, layout, torch, form, seed=0):
    R, state = _real(prec), J.STATES[name]
    vel = J.velocity(gsz, prec, seed)
    bases, views = _placed(layout, gsz, R, vel)
    dev = _on(torch, bases)
    ss = cz.set_rhs_div(*views(dev), scale=SCALE)
    assert cz.info()["field_form"] == form, (layout, cz.info()["field_form"])
    want, ss_ref = J.div(vel, state[1], SCALE, R)
    got = _rhs(cz, gsz, R)
    what = (gsz, name, layout, "device" if torch is not None else "numpy", form)
    if state[2]:  # the closed box: the mean the handle removed, then byte for byte with that mean
        inner = want[1:-1, 1:-1, 1:-1]
        m, _, B = CB.mean_of(inner, inner.size, R)
        mg = cz.closed_mean(0)
        assert abs(mg - float(m)) <= CB.mean_tol(m, B, inner.size), (what, mg, m)
        want[1:-1, 1:-1, 1:-1] = inner - R(mg)
    assert got.tobytes() == want.tobytes(), what
    assert abs(ss - ss_ref) <= 1e-12 * ss_ref, (what, ss, ss_ref)
    assert cz.set_rhs_div(*views(dev), scale=SCALE) == ss, what  # the same bits from run to run
    assert cz.set_rhs_div(*views(dev), scale=SCALE, want_norm=False) is None
    for a, b in zip(_back(dev), bases):
        assert a.tobytes() == b.tobytes(), what  # the velocity is only read


def _check_grad(cz, prec, gsz, name, layout, torch, form, seed=1):
    R, state = _real(prec), J.STATES[name]
    vel = J.velocity(gsz, prec, seed)
    for a, m in zip(vel, J.written(gsz, state[1])):
        a[~m] = KEEP
    _, p = PP.problem(gsz, prec, seed)
    cz.set_field(p)
    bases, views = _placed(layout, gsz, R, vel)
    dev = _on(torch, bases)
    cz.sub_grad(*views(dev), scale=SCALE)
    assert cz.info()["field_form"] == form, (layout, cz.info()["field_form"])
    new = J.sub_grad(vel, J.fill_field(p, state), state[1], SCALE, R)
    want, _ = _placed(layout, gsz, R, new)
    what = (gsz, name, layout, "device" if torch is not None else "numpy", form)
    for a, b in zip(_back(dev), want):
        assert a.tobytes() == b.tobytes(), what
    got = views(_back(dev))
    for ax in range(3):
        f = lambda c: tuple(c if d == ax else slice(1, -1) for d in range(3))  # noqa: E731
        if state[1][ax]:
            assert np.array_equal(got[ax][f(0)], got[ax][f(gsz[ax] - 2)]) and not (got[ax][f(0)] == KEEP).any(), what
        assert (got[ax][tuple(-1 if d == ax else slice(None) for d in range(3))] == KEEP).all(), what


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("check", [_check_div, _check_grad], ids=["set_rhs_div", "sub_grad"])
def test_bytes_in_every_layout_from_device_and_host(check, gsz, prec):
    """Dirichlet faces: C order, Fortran order, vel[..., 3] interleaved, a k-strided slice and a slice with k rows (odd phases), device
    tensors and numpy arrays; the row form where k is the unit stride, the generic form elsewhere"""
    torch = _torch()
    cz = _handle(prec, list(gsz) + SOLVER)
    try:
        for layout in LAYOUTS:
            for t in (torch, None):
                check(cz, prec, gsz, "dirichlet", layout, t, ROW_FORM[layout])
    finally:
        cz.close()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", SHAPES, ids=SHAPE_IDS)
def test_bytes_with_the_generic_form_forced(gsz, prec, monkeypatch):
    """CZ_FIELD_FORM=3: the generic kernels on the layouts the row form takes otherwise, in the states the box allows"""
    torch = _torch()
    monkeypatch.setenv("CZ_FIELD_FORM", "3")
    for name in ("dirichlet", "channel"):
        if not J.fits(gsz, J.STATES[name]):
            continue
        cz = _handle(prec, list(gsz) + SOLVER, J.STATES[name])
        try:
            for check in (_check_div, _check_grad):
                check(cz, prec, gsz, name, "c_order", torch, 3)
                check(cz, prec, gsz, name, "slice", None, 3)
        finally:
            cz.close()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", ["px", "channel", "closed", "triple", "inflow"])
def test_bytes_in_the_states(name, prec):
    """periodic X, the channel, the closed box (its mean against closed_mean(0)), the triply periodic box, an inflow plane: the seam reads
    face n - 1 for face 1 and writes face 1 with it; row form from device tensors, generic form from an interleaved numpy array"""
    torch = _torch()
    for gsz in SHAPES:
        if not J.fits(gsz, J.STATES[name]):
            continue
        cz = _handle(prec, list(gsz) + SOLVER, J.STATES[name])
        try:
            for check in (_check_div, _check_grad):
                check(cz, prec, gsz, name, "c_order", torch, 1)
                check(cz, prec, gsz, name, "slice", torch, 1)
                check(cz, prec, gsz, name, "interleaved", None, 3)
        finally:
            cz.close()


# ---- CZ.project end to end
def _count_bar(name, pc, coef, prec, rms0):
    """periodic_parity.COUNTS holds the iterations that take the seeded problem (b uniform in [-1e-2, 1e-2]: RMS 1e-2 / sqrt(3)) to an RMS
    residual of 1e-5; the test bars of DESIGN.md §5.15 allow 1.5 x such a count.  The projection asks for another reduction -- from the RMS
    of the divergence to eps -- so the bar is that count scaled by the ratio of the logarithms of the two reductions (the same mean
    reduction per iteration), times 1.5"""
    key = (name, pc, coef)
    if key not in P.COUNTS:
        return None
    asked = math.log(rms0 / J.E2E_EPS[prec]) / math.log(PP.B_SCALE / math.sqrt(3.0) / 1e-5)
    return math.ceil(1.5 * P.COUNTS[key] * asked)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", list(J.STATES))
@pytest.mark.parametrize("gsz", J.E2E_BOXES, ids=["x".join(map(str, g)) for g in J.E2E_BOXES])
def test_project_end_to_end(gsz, name, prec):
    """pcg mgrb 1.2 and mg 0.8 at eps 1e-10 (FP32: 1e-5): a second set_rhs_div gives ||div||_2 / ||div before||_2 within
    project_parity.BARS; the count is the restatement's, and within the scaled bar of periodic_parity.COUNTS where the state has one; closed
    states: the mean removed from the divergence of a velocity with zero wall velocities is at rounding level"""
    torch = _torch()
    R, state = _real(prec), J.STATES[name]
    vel = J.velocity(gsz, prec, 0, state)
    _, p0 = PP.problem(gsz, prec, 0)
    for pc, coef in J.E2E_RUNS:
        cz = _handle(prec, list(gsz) + ["pcg", 300, coef, pc], state)
        try:
            cz.set_eps(J.E2E_EPS[prec])
            cz.set_field(p0)
            t = [torch.from_numpy(a).cuda() for a in vel]
            itr, ss0 = cz.project(*t)
            m0 = cz.closed_mean(0)
            ss1 = cz.set_rhs_div(*t)
            ratio, (ref_ratio, ref_itr) = math.sqrt(ss1 / ss0), J.MEASURED[tuple(gsz), pc, name, prec]
            npts = int(np.prod([n - 2 for n in gsz]))
            bar = _count_bar(name, pc, coef, prec, math.sqrt(ss0 / npts))
            print(f"{gsz} {name} {prec} {pc}: ratio {ratio:.3e} (restatement {ref_ratio:.3e}, bar {J.BARS[name, prec]:.3e})  itr {itr} (restatement {ref_itr}, bar {bar})"
                  f"  mean of div {m0:.3e}")
            assert 0 < itr < 300 and ratio <= J.BARS[name, prec], (pc, ratio, J.BARS[name, prec])
            assert abs(itr - ref_itr) <= 1, (pc, itr, ref_itr)  # (the stopping residual may sit at either side of eps by the dots' rounding)
            assert bar is None or itr <= bar, (pc, itr, bar)
            if state[2]:
                # sum div = the net boundary flux = 0 exactly; a cell's d carries five roundings of at most half an ulp of a value below 8
                # (4 eps each), and the mean of the cells' errors is no larger than the largest: 20 eps, and the mean's own rounding
                assert abs(m0) <= 21.0 * float(np.finfo(R).eps), m0
            # the corrected velocity is the restatement's up to the solve's tolerance: its divergence is, see the ratio; face 0 = face n - 2
            got = [a.cpu().numpy() for a in t]
            for ax in range(3):
                if state[1][ax]:
                    f = lambda c: tuple(c if d == ax else slice(1, -1) for d in range(3))  # noqa: E731
                    assert np.array_equal(got[ax][f(0)], got[ax][f(gsz[ax] - 2)])
        finally:
            cz.close()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_closed_box_net_inflow_is_the_mean_removed(prec):
    """a closed box with a uniform inflow through X-: closed_mean(0) = flux / npts to 1e-12 relative (FP32: 1e-5)"""
    gsz, state = (33, 47, 61), J.STATES["closed"]
    vel = J.velocity(gsz, prec, 0, state, inflow=0.25)
    cz = _handle(prec, list(gsz) + SOLVER, state)
    try:
        cz.set_rhs_div(*vel)
        npts = int(np.prod([n - 2 for n in gsz]))
        want = math.fsum(J.div_raw(vel, state[1], _real(prec)).astype(np.float64).ravel()) / npts
        flux = J.boundary_flux(vel) / npts  # (out minus in: negative for an inflow)
        got = cz.closed_mean(0)
        print(f"{prec}: closed_mean(0) {got!r}, sum div / npts {want!r}, net flux / npts {flux!r}")
        tol = 1e-12 if prec == "f64" else 1e-5
        assert flux < 0.0 and abs(got - want) <= tol * abs(want) and abs(got - flux) <= tol * abs(flux)
    finally:
        cz.close()


# ---- the stream hand-over
def test_stream_hand_over_without_device_synchronisation():
    """a velocity produced on a side stream right before set_rhs_div (a large fill, then the final values) is read complete; without a norm
    the call does not wait; the corrected velocity is consumed on the caller's stream right after sub_grad"""
    torch = _torch()
    gsz, prec, state = (64, 64, 64), "f64", J.STATES["px"]
    vel = J.velocity(gsz, prec, 3)
    _, p0 = PP.problem(gsz, prec, 3)
    ref = _handle(prec, list(gsz) + SOLVER, state)
    try:
        ref.set_field(p0)
        want = [a.copy() for a in vel]
        want_itr, _ = ref.project(*want)
    finally:
        ref.close()
    cz = _handle(prec, list(gsz) + SOLVER, state)
    try:
        cz.set_field(p0)
        s = torch.cuda.Stream()
        host = [torch.from_numpy(a).pin_memory() for a in vel]
        junk = torch.empty(256 * 1024 * 1024 // 8, dtype=torch.float64, device="cuda")
        src = [torch.empty(gsz, dtype=torch.float64, device="cuda") for _ in range(3)]
        t = [torch.empty(gsz, dtype=torch.float64, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(8):
                junk.fill_(1.0)  # work in front of the final values, on the caller's stream
            for a, b, h in zip(src, t, host):
                a.fill_(123.0)
                a.copy_(h, non_blocking=True)
                b.copy_(h, non_blocking=True)
            assert cz.set_rhs_div(*src, want_norm=False) is None
            for a in src:
                a.fill_(0.0)  # the caller may reuse its arrays at once
            itr = cz.solve()
            cz.sub_grad(*t)
            doubled = [a * 2.0 for a in t]  # consumed on the caller's stream, no synchronisation before it
            out = [a.cpu() for a in doubled]
        assert itr == want_itr
        for a, b in zip(out, want):
            assert a.numpy().tobytes() == (b * 2.0).tobytes()
    finally:
        cz.close()


# ---- the refusals
def _raw(cz, fn, arrs, strides, on_device=0, scale=1.0):
    ptr = [C.c_void_p(a) if a is not None else None for a in arrs]
    st = (C.c_longlong * 3)(*strides) if strides is not None else None
    if fn == "cz_set_rhs_div":
        return cz.lib.cz_set_rhs_div(cz.h, *ptr, st, on_device, None, float(scale), None)
    return cz.lib.cz_sub_grad(cz.h, *ptr, st, on_device, None, float(scale))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_refusals_leave_the_arrays_and_the_rhs_alone(prec, capfd):
    from cubez_amd import CZ
    gsz, R = (9, 7, 12), _real(prec)
    vel = J.velocity(gsz, prec, 4)
    keep = [a.copy() for a in vel]
    ptrs = [a.ctypes.data for a in vel]
    st = [s // vel[0].itemsize for s in vel[0].strides]
    both = ("cz_set_rhs_div", "cz_sub_grad")
    fresh = CZ(prec, quiet=True)
    try:
        assert [_raw(fresh, fn, ptrs, st) for fn in both] == [0, 0]  # before cz_setup
    finally:
        fresh.close()
    n = {fn: 1 for fn in both}
    cz = _handle(prec, list(gsz) + SOLVER)
    try:
        b0, p0 = PP.problem(gsz, prec, 4)
        cz.set_rhs(b0)
        cases = [([None, ptrs[1], ptrs[2]], st, 0, 1.0), ([ptrs[0], ptrs[1], None], st, 0, 1.0), (ptrs, None, 0, 1.0),  # NULL
                 (ptrs, [0, st[1], st[2]], 0, 1.0), (ptrs, [st[0], -st[1], st[2]], 0, 1.0),  # a stride < 1
                 ([ptrs[0], ptrs[1] + 1, ptrs[2]], st, 0, 1.0),  # misaligned
                 (ptrs, st, 1, 1.0)]  # not memory of the device
        cases += [(ptrs, st, 0, s) for s in (0.0, -1.0, math.inf, math.nan)]
        if prec == "f32":
            cases += [(ptrs, st, 0, 1e-60), (ptrs, st, 0, 1e60)]  # not finite and positive as CZ_REAL
        for arrs, strides, on_dev, scale in cases:
            for fn in both:
                assert _raw(cz, fn, arrs, strides, on_dev, scale) == 0, (fn, arrs, strides, on_dev, scale)
                n[fn] += 1
        # cz_sub_grad alone: two cells of a component share an element; two components are one array
        assert _raw(cz, "cz_sub_grad", ptrs, [1, 1, 1]) == 0 and _raw(cz, "cz_sub_grad", [ptrs[0], ptrs[0], ptrs[2]], st) == 0
        n["cz_sub_grad"] += 2
        assert _raw(cz, "cz_set_rhs_div", [ptrs[0], ptrs[0], ptrs[2]], st) == 1  # (reading one array twice is harmless)
        cz.set_rhs(b0)
        with pytest.raises(ValueError):
            cz.set_rhs_div(vel[0], vel[1], np.asfortranarray(vel[2]))  # unequal strides
        with pytest.raises(ValueError):
            cz.sub_grad(vel[0], vel[1], vel[2][:, :, :-1])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(vel, keep))
        want = b0.copy()
        want[0], want[-1], want[:, 0], want[:, -1], want[:, :, 0], want[:, :, -1] = 0, 0, 0, 0, 0, 0
        assert _rhs(cz, gsz, R).tobytes() == want.tobytes()
    finally:
        cz.close()
    maf = _handle(prec, list(gsz) + ["jacobi_maf", 50, 0.8])
    try:
        assert [_raw(maf, fn, ptrs, st) for fn in both] == [0, 0]
        n = {fn: v + 1 for fn, v in n.items()}
    finally:
        maf.close()
    other = _handle(prec, list(gsz) + ["sor2sma", 50, 1.5])  # accepted on a handle of any other solver
    try:
        assert [_raw(other, fn, ptrs, st) for fn in both] == [1, 1]
    finally:
        other.close()
    err = capfd.readouterr().err
    assert {fn: err.count(fn + ":") for fn in both} == n, err
    for why in ("cz_setup first", "NULL pointer", "strides must be positive", "not aligned", "handle's device", "finite and positive", "share an element",
                "the same array", "MAF"):
        assert why in err, why


def test_a_decomposed_run_is_refused(capfd):
    """(2, 1, 1) on the LOCAL transport: both entries return 0 on every rank, with the line that names the follow-up"""
    gsz = (32, 36, 40)

    def work(q):
        cz = _handle("f32", list(gsz) + ["pcg", 10, 0.8, "jacobi", 2, 1, 1])
        try:
            vel = [np.ones(tuple(cz.local()["size"]), dtype=np.float32) for _ in range(3)]
            ptrs = [a.ctypes.data for a in vel]
            st = [s // 4 for s in vel[0].strides]
            before = cz.field()
            out = (_raw(cz, "cz_set_rhs_div", ptrs, st), _raw(cz, "cz_sub_grad", ptrs, st))
            return out, bool(all((a == 1).all() for a in vel)), cz.field().tobytes() == before.tobytes()
        finally:
            cz.close()

    assert TN._ranks("f32", (2, 1, 1), work) == [((0, 0), True, True)] * 2
    err = capfd.readouterr().err
    assert err.count("exchange of one velocity layer") == 4 and err.count("follow-up") == 4, err
