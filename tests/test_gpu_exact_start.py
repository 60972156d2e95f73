"""pcg on exact starts and on scaled problems on the GPU (-m gpu).

An exact start (tests/exact_start.py: b = 0 with p = 0, or integer data with b = A p) has an initial residual of zero in every bit.  The
solve must stop at iteration 1 before it touches the field: cz_solve returns 0, get_field returns the bytes it returned before, the history
is empty, the residual 0, info()["void_start"] 1 -- with every preconditioner, whose rho the host learns only after the iteration's
launches.  The restatements do the same (tests/test_exact_start_oracle.py).  CZ.project on a velocity that is already divergence-free
goes that way: the velocity keeps its bytes.  A scaled problem (p, b) * 2^-s gives the field and the history of (p, b) times 2^-s bit for bit
(GPU against GPU: the same launches, the same summation order) until rho falls under the absolute threshold, from exact_start.FIRST_STOP on.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_start as X  # noqa: E402
import problem_parity as PP  # noqa: E402
import test_gpu_neumann as TN  # noqa: E402
from test_gpu_periodic import _handle  # noqa: E402
from test_gpu_problem import _torch  # noqa: E402

pytestmark = pytest.mark.gpu
BOX_IDS = ["x".join(map(str, g)) for g in X.BOXES]
ITR_AFTER = 6  # the ordinary solve that follows: at most this many iterations


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """torch's HIP runtime up before the library is loaded, the order of tests/test_gpu_walk.py and bench.py: the tests of this file that hand
    over device tensors would otherwise find no device when the file runs alone"""
    _torch().cuda.init()


def _args(gsz, pc, itr_max=ITR_AFTER, div=None):
    return list(gsz) + ["pcg", itr_max, X.COEF, pc] + (list(div) if div else [])


def _stopped_untouched(cz, what):
    """solve on the start the handle holds: the contract of an exact start.  Returns the field"""
    before = cz.get_field()
    itr = cz.solve()
    after = cz.get_field()
    assert itr == 0 and cz.iter == 0, (what, itr, cz.iter)
    assert after.tobytes() == before.tobytes(), (what, "the field changed", int(np.isnan(after).sum()), "NaN")
    assert cz.history() == [] and cz.res == 0.0, (what, cz.history(), cz.res)
    assert cz.info()["void_start"] == 1, what
    return after


def _ordinary(cz, gsz, prec, sl=None):
    """the seeded problem on the handle: (itr, history, field)"""
    b, p = PP.problem(gsz, prec, 1)
    sl = sl if sl is not None else (slice(None),) * 3
    cz.set_rhs(b[sl])
    cz.set_field(p[sl])
    itr = cz.solve()
    assert itr > 0 and cz.info()["void_start"] == 0
    return itr, cz.history(), cz.get_field()


@pytest.mark.parametrize("name", list(X.STATES))
@pytest.mark.parametrize("pc", X.PCS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz", X.BOXES, ids=BOX_IDS)
def test_exact_start_stops_before_it_touches_the_field(gsz, prec, pc, name):
    """both kinds of start through set_rhs / set_field / solve / get_field, then an ordinary solve on the same handle against a fresh twin's"""
    state = X.STATES[name]
    cz, twin = _handle(prec, _args(gsz, pc), state), _handle(prec, _args(gsz, pc), state)
    try:
        for kind in X.KINDS:
            b, p = X.start(gsz, prec, state, kind)
            cz.set_rhs(b)
            cz.set_field(p)
            got = _stopped_untouched(cz, (gsz, prec, pc, name, kind))
            assert got.tobytes() == p.tobytes(), (gsz, prec, pc, name, kind)
        mine, fresh = _ordinary(cz, gsz, prec), _ordinary(twin, gsz, prec)
        assert mine[0] == fresh[0] and mine[1] == fresh[1] and mine[2].tobytes() == fresh[2].tobytes(), (gsz, prec, pc, name)
    finally:
        cz.close()
        twin.close()


@pytest.mark.parametrize("pc", ["jacobi", "mg"])
def test_exact_start_with_the_unfused_update(pc, monkeypatch):
    """CZ_CG_FUSE=0: the triads carry no test of their own, the host learns rho before them"""
    monkeypatch.setenv("CZ_CG_FUSE", "0")
    gsz, prec = X.BOXES[0], "f64"
    cz = _handle(prec, _args(gsz, pc))
    try:
        assert cz.config_in_force()["cg_fuse"] == 0
        for kind in X.KINDS:
            b, p = X.start(gsz, prec, X.STATES["dirichlet"], kind)
            cz.set_rhs(b)
            cz.set_field(p)
            _stopped_untouched(cz, (pc, kind, "unfused"))
    finally:
        cz.close()


def test_exact_start_decomposed():
    """pcg mg, FP64, (2, 1, 1) on the LOCAL transport, ranks as threads: every rank stops alike, and the ordinary solve that follows equals
    that of ranks that made no exact start"""
    _torch().cuda.init()  # (torch's runtime before the library's, as tests/test_gpu_walk.py)
    from cubez_amd import CZ
    gsz, prec, div = (32, 36, 40), "f64", (2, 1, 1)
    state = X.STATES["dirichlet"]

    def work(exact):
        def rank(q):
            cz = CZ(prec, quiet=True)
            assert cz.setup(_args(gsz, "mg", div=div)) == 1
            sl = cz.global_slice()
            if exact:
                for kind in X.KINDS:
                    b, p = X.start(gsz, prec, state, kind)
                    cz.set_rhs(b[sl])
                    cz.set_field(p[sl])
                    _stopped_untouched(cz, ("decomposed", q, kind))
            out = _ordinary(cz, gsz, prec, sl)
            cz.close()
            return out
        return rank

    mine, fresh = TN._ranks(prec, div, work(True)), TN._ranks(prec, div, work(False))
    for a, b in zip(mine, fresh):
        assert a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("pc", X.PCS)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_project_leaves_a_divergence_free_velocity_alone(prec, pc):
    """a fluid at rest and a discrete curl of integers, from device tensors and from numpy arrays: (0, 0.0), the velocity bit-identical, the
    field in the handle finite"""
    torch = _torch()
    R = X.real(prec)
    for gsz in X.BOXES:
        cz = _handle(prec, _args(gsz, pc))
        try:
            for vel in ([np.zeros(gsz, dtype=R) for _ in range(3)], X.divergence_free(gsz, prec)):
                for on_device in (True, False):
                    what = (gsz, prec, pc, bool(vel[0].any()), on_device)
                    cz.set_field(np.zeros(gsz, dtype=R))
                    arrays = [torch.from_numpy(v.copy()).cuda() if on_device else v.copy() for v in vel]
                    itr, ss = cz.project(*arrays)
                    assert (itr, ss) == (0, 0.0) and cz.info()["void_start"] == 1, (what, itr, ss)
                    for a, v in zip(arrays, vel):
                        a = a.cpu().numpy() if on_device else a
                        assert a.tobytes() == v.tobytes(), (what, "the velocity changed", int(np.isnan(a).sum()), "NaN")
                    f = cz.get_field()
                    assert np.isfinite(f).all() and not f.any(), what
        finally:
            cz.close()


def test_refined_solve_on_an_exact_start():
    """ss0 == 0: no step, no exception, the FP64 field bit-identical"""
    _torch()
    from cubez_amd.refine import Refined
    gsz = X.BOXES[0]
    b, p = X.start(gsz, "f64", X.STATES["dirichlet"], "integers")
    r = Refined(gsz)
    try:
        r.set_rhs(b)
        r.set_field(p)
        before = r.get_field()
        assert r.solve() == 0 and r.history == []
        assert r.get_field().tobytes() == before.tobytes() == p.tobytes()
    finally:
        r.close()


# ---- scaling
def _scaled(cz, prec, s, base):
    b, p = X.scaled_problem(prec, s, base)
    cz.set_rhs(b)
    cz.set_field(p)
    before = cz.get_field()
    itr = cz.solve()
    return itr, cz.history(), cz.get_field(), before


@pytest.mark.parametrize("prec,pc", list(X.SCALED), ids=[f"{q}_{pc}" for q, pc in X.SCALED])
def test_k_iterations_scale_bit_for_bit(prec, pc):
    """eps below reach, so exactly K iterations run: the field and the history of (p, b) * 2^-s are those of (p, b) times 2^-s"""
    base = X.builtin_problem(prec)
    cz = _handle(prec, _args(X.SCALE_BOX, pc, X.SCALE_K))
    try:
        cz.set_eps(X.EPS_BELOW_REACH)
        itr0, h0, f0, _ = _scaled(cz, prec, 0, base)
        assert itr0 == X.SCALE_K and len(h0) == X.SCALE_K
        for s in X.SCALED[prec, pc]:
            f = 2.0 ** -s
            itr, h, field, _ = _scaled(cz, prec, s, base)
            assert itr == X.SCALE_K, (prec, pc, s, itr)
            assert field.tobytes() == (f0 * f0.dtype.type(f)).tobytes(), (prec, pc, s)
            assert h == [v * f for v in h0], (prec, pc, s)
    finally:
        cz.close()


@pytest.mark.parametrize("prec,pc", list(X.FIRST_STOP), ids=[f"{q}_{pc}" for q, pc in X.FIRST_STOP])
def test_beyond_the_threshold_the_solve_stops_with_the_field_untouched(prec, pc):
    """the threshold |rho| < FLT_MIN is absolute in both precisions: the restatement's first s that stops (exact_start.FIRST_STOP: 68 for none
    and jacobi, 69 for mg and mgrb, FP32 and FP64 alike) is the GPU's, and s = 70 stops (exact_start.STOPS).  One less makes iteration 1 and
    breaks down at iteration 2 (on the restatement rho is 1.08 to 3.5 thresholds at iteration 1 and 0.06 to 0.17 at iteration 2): the field is
    then that of iteration 1, bit for bit -- a breakdown at a later iteration does not touch the field either"""
    base = X.builtin_problem(prec)
    first = X.FIRST_STOP[prec, pc]
    cz = _handle(prec, _args(X.SCALE_BOX, pc, X.SCALE_K))
    try:
        cz.set_eps(X.EPS_BELOW_REACH)
        cz.set_itr_max(1)
        itr, h1, f1, _ = _scaled(cz, prec, first - 1, base)
        assert itr == 1 and len(h1) == 1 and math.isfinite(h1[0]) and h1[0] > 0.0, (prec, pc, first - 1, itr, h1)
        cz.set_itr_max(X.SCALE_K)
        itr, h, field, _ = _scaled(cz, prec, first - 1, base)
        assert itr == 0 and h == h1 and cz.info()["void_start"] == 0, (prec, pc, first - 1, itr, h, h1)
        assert field.tobytes() == f1.tobytes(), (prec, pc, first - 1, "the field of iteration 1 changed", int(np.isnan(field).sum()), "NaN")
        for s in sorted({first, first + 1, X.STOPS.get((prec, pc), first)}):
            itr, h, field, before = _scaled(cz, prec, s, base)
            assert itr == 0 and h == [] and cz.res == 0.0 and cz.info()["void_start"] == 1, (prec, pc, s, itr)
            assert field.tobytes() == before.tobytes(), (prec, pc, s)
    finally:
        cz.close()
