"""The one boundary state and the one fill on the GPU (-m gpu; cz_bc.h): czhip_mirror_faces_async as the fill with kinds
0 / 1, and a library-level hierarchy whose two setters each replace their half of one state."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neumann_parity as N  # noqa: E402
import periodic_parity as P  # noqa: E402
import test_gpu_neumann as TN  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
G = O.GUIDE
OMG = {"mg": 0.8, "mgrb": 1.2}


def _random(hip, gsz, seed):
    return np.random.default_rng(seed).random((gsz[1] + 2 * G, gsz[0] + 2 * G, gsz[2] + 2 * G)).astype(hip.real)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_mirror_takes_any_non_zero_flag_as_set(prec):
    """flags (2, 0, 0, 5, 0, -1) are the mask (1, 0, 0, 1, 0, 1): byte for byte the mirror of the restatement, in one launch -- the wrapper
    neither takes a flag for the fill's wrap (2) nor refuses one that is no kind (5, -1)"""
    from cubez_amd.lib import CzHip
    hip = CzHip(prec)
    gsz = (9, 7, 12)
    sz, idx = TN._box(gsz)
    host = _random(hip, gsz, 41)
    d = hip.alloc(sz, host)
    try:
        hip.timing(True)
        assert hip.mirror_faces(d, sz, idx, (2, 0, 0, 5, 0, -1))
        want = N.mirror(host.copy(), sz, idx, (1, 0, 0, 1, 0, 1))
        assert not np.array_equal(want, host)
        assert d.get().tobytes() == want.tobytes()
        assert hip.timing_read("bc_mirror")[0] == 1
    finally:
        hip.timing(False)
        hip.sync()
        d.free()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("mask", list(TN.MIRROR_MASKS))
@pytest.mark.parametrize("gsz", [(9, 7, 12), (33, 47, 61)], ids=["9x7x12", "33x47x61"])
def test_mirror_is_the_fill_with_kinds_0_and_1(gsz, mask, prec):
    """czhip_mirror_faces_async(faces) and czhip_fill_faces_async(kinds of faces, no periodic direction) leave byte-equal arrays and count equal
    launches, on the whole box and on a brick whose - sides are rank-internal"""
    from cubez_amd.lib import CzHip
    hip = CzHip(prec)
    faces = TN.MIRROR_MASKS[mask]
    sz, idx = TN._box(gsz)
    idx_b = [1, idx[1], 1, idx[3], 1, idx[5]]
    host = _random(hip, gsz, 42)
    d = hip.alloc(sz, host)
    try:
        out, launches = {}, {}
        for name, call in (("mirror", lambda ix: hip.mirror_faces(d, sz, ix, faces)), ("fill", lambda ix: hip.fill_faces(d, sz, ix, P.kinds(faces, P.NOPER)))):
            hip.timing(True)
            out[name] = []
            for ix in (idx, idx_b):
                d.put(host)
                assert call(ix)
                out[name].append(d.get().tobytes())
            launches[name] = hip.timing_read("bc_mirror")[0]
            hip.timing(False)
        assert out["mirror"] == out["fill"]
        assert out["mirror"][0] != host.tobytes()
        assert launches["mirror"] == launches["fill"] == 1 + int(any(faces[f] for f in (1, 3, 5)))
    finally:
        hip.timing(False)
        hip.sync()
        d.free()


def _apply(hip, h, dz, dr, omg, calls):
    """z of the hierarchy after the setter calls (("neumann" | "periodic", argument), ...) in their order; z's face layers are the caller's to
    keep zero on Dirichlet faces, so z starts as zeros each time"""
    for which, arg in calls:
        assert (hip.mg_set_neumann if which == "neumann" else hip.mg_set_periodic)(h, arg)
    dz.put(np.zeros(dz.shape, dtype=hip.real))
    assert hip.mg_apply(h, dz, dr, omg)
    return dz.get()


# (12, 4, 9): two inner points in Y, one at every level >= 1 -- the one-point case of mg_level_bc.  ((9, 7, 12) has 5, 3 and 2 points in Y)
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("kind", ["mg", "mgrb"])
@pytest.mark.parametrize("gsz", [(9, 7, 12), (12, 4, 9)], ids=["9x7x12", "12x4x9"])
def test_hierarchy_setters_each_replace_their_half_of_one_state(gsz, kind, prec):
    """czhip_mg_set_neumann(five faces) then czhip_mg_set_periodic(Y), the reverse order on a fresh hierarchy, and the reverse order again after
    an unrelated state (periodic Z, mask X-) with a cycle under it: czhip_mg_apply_async gives the same bytes for the same r, those of the
    restatement -- no half of the state is stale, none is lost when the other is set"""
    from cubez_amd.lib import CzHip
    hip = CzHip(prec)
    sz, idx, ins, r = TN._cycle_rhs(prec, gsz)
    five, py = ("neumann", N.FIVE), ("periodic", P.PY)
    ref = P.apply(kind, P.kernels(prec, N.FIVE, P.PY), r, sz, idx, OMG[kind])[ins]
    create = hip.mg_create_rb if kind == "mgrb" else hip.mg_create
    h1, h2 = create(sz, idx), create(sz, idx)
    assert h1 and h2
    dr, dz = hip.alloc(sz, r), hip.alloc(sz, np.zeros_like(r))
    try:
        z1 = _apply(hip, h1, dz, dr, OMG[kind], [five, py])
        z2 = _apply(hip, h2, dz, dr, OMG[kind], [py, five])
        other = _apply(hip, h1, dz, dr, OMG[kind], [("periodic", P.PZ), ("neumann", N.X_MINUS)])
        z3 = _apply(hip, h1, dz, dr, OMG[kind], [py, five])
        z4 = _apply(hip, h2, dz, dr, OMG[kind], [("neumann", N.X_MINUS), ("periodic", P.PZ), five, py])
        assert z1[ins].tobytes() == ref.tobytes()
        assert other[ins].tobytes() != z1[ins].tobytes()
        for z in (z2, z3, z4):
            assert z[ins].tobytes() == z1[ins].tobytes()
    finally:
        hip.sync()
        hip.mg_destroy(h1), hip.mg_destroy(h2)
        dr.free(), dz.free()
