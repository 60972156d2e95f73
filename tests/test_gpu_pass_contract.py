"""GPU tests (-m gpu) of the convergence contract of every checked launch (include/cz_hip.h, part 3): the last workgroup of a checked sweep
or pass writes sqrt(sum * res_normal) to hist[itr + s] for its sweeps in order, stops at the first one below eps and then sets the flag and
conv_itr; a launch that finds the flag (or a separate skip flag) set does nothing at all; czhip_check_async / czhip_check2_async do the
same bookkeeping on sums that are already on the device.  The sums come from the oracle's wide (double) accumulation, eps is placed between
two residuals with a relative margin of at least 1e-6, so that no summation order can move the converged sweep."""
import numpy as np
import pytest

from oracle import cz_oracle as O

pytestmark = pytest.mark.gpu

# small boxes of the kernel tests' lists (T2_BOXES of test_gpu_kernels.py, BOXES of test_gpu_jac3.py): an index range that includes the
# faces, rows that are no multiple of the vector width, and rows cut into k windows
BOXES = [((24, 20, 28), (1, 24, 1, 20, 1, 28)), ((40, 36, 61), None), ((9, 7, 1100), None)]
BOX_IDS = ["24x20x28_idx", "40x36x61", "9x7x1100"]

# entry point -> sweeps (iterations) per launch
SWEEPS = {"jacobi": 1, "rbsor": 1, "jacobi2": 2, "rbsor2": 1, "rbsor4": 2, "jacobi3": 3, "jacobi4": 4}
# the launch forms each entry can be forced into: pair (threads, vectors, planes per chunk, k window), rb4 / jac3 / jac4 (k window, planes)
PAIR_FORMS = [(-2, 2, 0, -1), (512, 2, 5, 6), (1024, 2, 11, 17)]
DEEP_FORMS = [(0, 0), (5, 0), (9, 3)]
FORMS = {"jacobi": [None], "rbsor": [None], "jacobi2": PAIR_FORMS, "rbsor2": PAIR_FORMS, "rbsor4": DEEP_FORMS, "jacobi3": DEEP_FORMS,
         "jacobi4": DEEP_FORMS}

OMG = {"jacobi": 0.9, "jacobi2": 0.9, "jacobi3": 0.9, "jacobi4": 0.9, "rbsor": 1.3, "rbsor2": 1.3, "rbsor4": 1.3}
ITR = 7                # iteration number of the launch's first sweep
NH = 16                # history entries on the device
HSENT = -3.25          # sentinel of the history
CSENT = -77            # sentinel of conv_itr
MARGIN = 1e-6


def _hip(prec):
    from cubez_amd import CzHip
    return CzHip(prec)


def _set_form(h, kind, form):
    if form is None:
        return
    if kind in ("jacobi2", "rbsor2"):
        tb, mv, tj, win = form
        assert h.set_tuning2(tb, mv, tj, 1)
        h.lib.czhip_set_pair_window(win)
    elif kind == "rbsor4":
        assert h.lib.czhip_set_rb4(2, *form) == 0
    elif kind == "jacobi3":
        assert h.lib.czhip_set_jac3(2, *form) == 0
    else:
        assert h.lib.czhip_set_jac4(2, *form) == 0


def _reset_forms(h):
    h.set_tuning2(-2, 2, 0, 1)
    h.lib.czhip_set_pair_window(-1)
    h.lib.czhip_set_rb4(1, 0, 0)
    h.lib.czhip_set_jac3(1, 0, 0)
    h.lib.czhip_set_jac4(1, 0, 0)


def _problem(prec, box, kind):
    """random field and right-hand side, diagonally dominant coefficients (the residuals fall from sweep to sweep); the oracle's field after
    all sweeps of the launch and the wide sum of every sweep (iteration)"""
    (ni, nj, nk), idx = box
    sz = [ni, nj, nk]
    idx = list(idx) if idx else [2, ni - 1, 2, nj - 1, 2, nk - 1]
    ko = O.Kernels("oracle", prec)
    R = ko.real
    rng = np.random.default_rng(ni + 3 * nj + 5 * nk + 7 * len(kind))
    shape = (nj + 4, ni + 4, nk + 4)
    cf = rng.uniform(0.6, 1.0, 7).astype(R)
    cf[6] = 6.2
    p, b = (rng.uniform(-1, 1, shape).astype(R) for _ in range(2))
    a, wk, sums = p.copy(), np.zeros_like(p), []
    for _ in range(SWEEPS[kind]):
        wide = np.zeros(1)
        if kind.startswith("jacobi"):
            ko.jacobi(a, sz, idx, cf, OMG[kind], b, wk, wide=wide)
        else:
            for color in (0, 1):
                ko.psor2sma_core(a, sz, idx, cf, 0, color, OMG[kind], b, wide=wide)
        sums.append(float(wide[0]))
    npts = (idx[1] - idx[0] + 1) * (idx[3] - idx[2] + 1) * (idx[5] - idx[4] + 1)
    return sz, idx, cf, p, b, a, np.array(sums), 1.0 / npts


def _eps_for(res, t):
    """eps such that sweep t (1-based) is the first below it; t = 0: none is.  Every residual at least MARGIN (relative) away from eps."""
    if t == 0:
        eps = res.min() / 1.01
    elif t == 1:
        eps = res[0] * 1.5
    else:
        lo, hi = res[t - 1], res[:t - 1].min()
        assert lo * (1 + 4 * MARGIN) < hi, f"residuals do not fall: {res}"
        eps = np.sqrt(lo * hi)
    assert all(abs(r - eps) >= MARGIN * eps for r in res), (res, eps)
    return eps


def _launch(h, kind, dp, dw, db, sz, idx, cf, ck):
    """one checked launch of `kind`; returns launched.  rbsor: colour 0 (skip = the flag), then colour 1 with the check, in place on dp."""
    if kind == "jacobi":
        h.jacobi_checked(dp, dw, db, sz, idx, cf, OMG[kind], ck)
        return True
    if kind == "rbsor":
        h.rbsor_async(dp, db, sz, idx, cf, 0, 0, OMG[kind], ck["res"], 0, ck["flag"] if ck.get("hist") is not None else ck.get("skip"))
        if ck.get("hist") is None:
            h.rbsor_async(dp, db, sz, idx, cf, 0, 1, OMG[kind], ck["res"], 1, ck.get("skip"))
        else:
            h.rbsor_checked(dp, db, sz, idx, cf, 0, 1, OMG[kind], 1, ck)
        return True
    return h.pass_checked(kind, dp, dw, db, sz, idx, cf, OMG[kind], ck)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _state(h, flag=0, conv=CSENT, res_fill=0.0):
    return dict(res=h.dbuf(4, np.float64, res_fill), hist=h.dbuf(NH, np.float64, HSENT), flag=h.dbuf(1, np.int32, flag),
                conv=h.dbuf(1, np.int32, conv))


def _free(*bufs):
    for d in bufs:
        if d is not None:
            d.free()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("box", BOXES, ids=BOX_IDS)
@pytest.mark.parametrize("kind", list(SWEEPS))
def test_checked_launch_bookkeeping_against_wide_oracle(kind, box, prec):
    """For every landing -- no sweep, or sweep 1, 2, 3, 4 of the launch first below eps -- and every forced form: the sums of all sweeps, hist
    of every sweep up to the converged one (later entries keep their sentinel: the bookkeeping stops there), flag and conv_itr = the first
    converged sweep, the field after ALL sweeps of the launch bit for bit, the input untouched."""
    h = _hip(prec)
    sz, idx, cf, p, b, want, sums, rn = _problem(prec, box, kind)
    res = np.sqrt(sums * rn)
    n = SWEEPS[kind]
    db = h.alloc(sz, b)
    launched = 0
    try:
        for form in FORMS[kind]:
            _set_form(h, kind, form)
            for t in range(n + 1):
                eps = _eps_for(res, t)
                st = _state(h)
                ck = dict(st, res_normal=rn, eps=eps, itr=ITR)
                dp, dw = h.alloc(sz, p), h.alloc(sz, p)
                try:
                    if not _launch(h, kind, dp, dw, db, sz, idx, cf, ck):
                        continue
                    launched += 1
                    what = (form, t)
                    got = st["res"].get()
                    if kind == "rbsor":
                        assert _rel(got[0], sums[0]) < 1e-11, what
                    else:
                        for s in range(n):
                            assert _rel(got[s], sums[s]) < 1e-11, (what, s, got[s], sums[s])
                    hist = st["hist"].get()
                    last = t if t else n  # sweeps whose residual is recorded
                    for s in range(last):
                        assert _rel(hist[ITR + s], res[s]) < 1e-11, (what, s, hist[ITR + s], res[s])
                    rest = [i for i in range(NH) if not ITR <= i < ITR + last]
                    assert (hist[rest] == HSENT).all(), (what, hist)
                    assert int(st["flag"].get()[0]) == (1 if t else 0), what
                    assert int(st["conv"].get()[0]) == (ITR + t - 1 if t else CSENT), what
                    if kind != "rbsor":  # out of place
                        assert dw.get().tobytes() == want.tobytes(), what
                        assert dp.get().tobytes() == p.tobytes(), what
                    else:
                        assert dp.get().tobytes() == want.tobytes(), what
                finally:
                    _free(dp, dw, *st.values())
    finally:
        _reset_forms(h)
        db.free()
    fused = kind not in ("jacobi", "rbsor")
    if kind == "jacobi4" and prec == "f64":  # (jac4_k is built for FP32 only: the launcher declines every form)
        assert launched == 0
    elif not (fused and box[1] is not None):  # (the fused passes leave an index range that includes the faces to the single sweeps)
        assert launched == len(FORMS[kind]) * (n + 1)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("box", BOXES, ids=BOX_IDS)
@pytest.mark.parametrize("kind", list(SWEEPS))
def test_launch_after_convergence_changes_nothing(kind, box, prec):
    """A launch queued after convergence: the flag was set (conv_itr = 3, an earlier iteration) before it.  Destination, field, res slots,
    hist, flag and conv_itr stay byte for byte what they were, in every form.  Also the skip-only use of the fused passes (hist NULL, a separate
    skip flag, as decomposed runs call them): set, nothing changes; clear, the sums are written and hist, flag, conv_itr are not touched."""
    h = _hip(prec)
    sz, idx, cf, p, b, want, sums, rn = _problem(prec, box, kind)
    fused = kind not in ("jacobi", "rbsor")
    junk = np.full_like(p, 7.25)
    db = h.alloc(sz, b)
    try:
        for form in FORMS[kind]:
            _set_form(h, kind, form)
            # the flag doubles as the skip flag
            st = _state(h, flag=1, conv=3, res_fill=1.5e300)
            dp, dw = h.alloc(sz, p), h.alloc(sz, junk)
            try:
                _launch(h, kind, dp, dw, db, sz, idx, cf, dict(st, res_normal=rn, eps=1e30, itr=ITR))
                assert dp.get().tobytes() == p.tobytes() and dw.get().tobytes() == junk.tobytes(), form
                assert (st["res"].get() == 1.5e300).all() and (st["hist"].get() == HSENT).all(), form
                assert int(st["flag"].get()[0]) == 1 and int(st["conv"].get()[0]) == 3, form
            finally:
                _free(dp, dw, *st.values())
            if not fused and kind != "rbsor":
                continue
            for skip_set in (1, 0):
                st = _state(h, flag=0, res_fill=1.5e300)
                skip = h.dbuf(1, np.int32, skip_set)
                dp, dw = h.alloc(sz, p), h.alloc(sz, junk if kind != "rbsor" else p)
                try:
                    ck = dict(st, hist=None, skip=skip, res_normal=rn, eps=1e30, itr=ITR)
                    ok = _launch(h, kind, dp, dw, db, sz, idx, cf, ck)
                    if kind == "jacobi4" and prec == "f64":  # (FP32 only: declined, so nothing may be written -- the branch below)
                        assert not ok, form
                    assert (st["hist"].get() == HSENT).all() and int(st["flag"].get()[0]) == 0, (form, skip_set)
                    assert int(st["conv"].get()[0]) == CSENT and int(skip.get()[0]) == skip_set, (form, skip_set)
                    if skip_set or not ok:
                        assert dp.get().tobytes() == p.tobytes() and (st["res"].get() == 1.5e300).all(), (form, skip_set)
                        if kind != "rbsor":
                            assert dw.get().tobytes() == junk.tobytes(), (form, skip_set)
                    else:
                        got = st["res"].get()
                        if kind in ("rbsor", "rbsor2"):
                            assert _rel(got[0], sums[0]) < 1e-11, form
                        else:
                            assert all(_rel(got[s], sums[s]) < 1e-11 for s in range(SWEEPS[kind])), (form, got, sums)
                        assert (dp if kind == "rbsor" else dw).get().tobytes() != (p if kind == "rbsor" else junk).tobytes()
                finally:
                    _free(dp, dw, skip, *st.values())
    finally:
        _reset_forms(h)
        db.free()


# -- czhip_check_async / czhip_check2_async on crafted sums
def _check(h, sums, rn, eps, itr=5, flag=0, conv=CSENT):
    pair = len(sums) == 2
    st = _state(h, flag=flag, conv=conv)
    try:
        st["res"].put(np.array(list(sums) + [0.0] * (4 - len(sums))))
        h.check(dict(st, res_normal=rn, eps=eps, itr=itr), pair=pair)
        return st["hist"].get(), int(st["flag"].get()[0]), int(st["conv"].get()[0])
    finally:
        _free(*st.values())


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_check_below_above_equal_and_already_set(prec):
    """res = sqrt(sum * res_normal) < eps (strictly) sets the flag and conv_itr once; sqrt(4 * 1) = 2 is exact, so res == eps must not
    converge whatever the rounding of sqrt; an already set flag leaves everything alone."""
    h = _hip(prec)
    hist, flag, conv = _check(h, [2.25], 1.0, 2.0)                 # 1.5 < 2
    assert hist[5] == 1.5 and flag == 1 and conv == 5
    assert (np.delete(hist, 5) == HSENT).all()
    hist, flag, conv = _check(h, [2.25], 1.0, 1.0)                 # 1.5 > 1
    assert hist[5] == 1.5 and flag == 0 and conv == CSENT
    hist, flag, conv = _check(h, [4.0], 1.0, 2.0)                  # 2 == 2: not below
    assert hist[5] == 2.0 and flag == 0 and conv == CSENT
    hist, flag, conv = _check(h, [4.0], 1.0, np.nextafter(2.0, 3.0))  # one ulp above: below
    assert hist[5] == 2.0 and flag == 1 and conv == 5
    hist, flag, conv = _check(h, [2.25], 1.0, 2.0, flag=1, conv=3)  # converged earlier
    assert (hist == HSENT).all() and flag == 1 and conv == 3


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_check2_first_second_neither_equal_and_already_set(prec):
    """The pair check: the first sum converging stops there (hist of the second sweep keeps its sentinel, conv_itr = itr); the second
    converging gives conv_itr = itr + 1; equality converges on neither; an already set flag leaves everything alone."""
    h = _hip(prec)
    hist, flag, conv = _check(h, [1.0, 100.0], 1.0, 2.0)
    assert hist[5] == 1.0 and hist[6] == HSENT and flag == 1 and conv == 5
    hist, flag, conv = _check(h, [100.0, 1.0], 1.0, 2.0)
    assert hist[5] == 10.0 and hist[6] == 1.0 and flag == 1 and conv == 6
    hist, flag, conv = _check(h, [100.0, 64.0], 1.0, 2.0)
    assert hist[5] == 10.0 and hist[6] == 8.0 and flag == 0 and conv == CSENT
    hist, flag, conv = _check(h, [4.0, 4.0], 1.0, 2.0)
    assert hist[5] == 2.0 and hist[6] == 2.0 and flag == 0 and conv == CSENT
    hist, flag, conv = _check(h, [1.0, 1.0], 1.0, 2.0, flag=1, conv=3)
    assert (hist == HSENT).all() and flag == 1 and conv == 3
    assert (np.delete(_check(h, [100.0, 1.0], 1.0, 2.0)[0], [5, 6]) == HSENT).all()


def test_device_sqrt_of_the_check_is_correctly_rounded():
    """hist = sqrt(sum * res_normal) of the device equals numpy's (IEEE, correctly rounded) bit for bit on sums and normalisations of
    every magnitude the solvers produce."""
    h = _hip("f64")
    rng = np.random.default_rng(11)
    sums = np.concatenate([10.0 ** rng.uniform(-30, 10, 24), rng.uniform(0.5, 2.0, 8)])
    for s in sums:
        rn = 1.0 / float(rng.integers(1, 1 << 27))
        hist, _, _ = _check(h, [s], rn, 0.0)
        want = np.sqrt(np.float64(s) * np.float64(rn))
        assert hist[5].tobytes() == want.tobytes(), (s, rn, hist[5], want)
        hist, _, _ = _check(h, [1e300, s], rn, 0.0)
        assert hist[6].tobytes() == want.tobytes(), (s, rn, hist[6], want)
