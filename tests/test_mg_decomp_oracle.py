"""The distributed V-cycle of `pcg ... mg` on the CPU (DESIGN.md §5.10 "Decomposed runs"): the ownership rule of the coarse points
(cubez_amd.decomp.mg_own, restating comm_mg_own), the gather level, and a numpy restatement of the brick-wise cycle -- every brick computes on
its owned points only, its ghost cells filled by slicing what the neighbours own -- against tests/mg_parity.vcycle, bit for bit."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_parity as M  # noqa: E402
from cubez_amd import decomp as D  # noqa: E402

DIVS = [(2, 1, 1), (1, 2, 1), (1, 1, 2), (2, 2, 2), (3, 1, 2), (1, 3, 3), (3, 3, 1), (4, 1, 1), (2, 3, 1)]
SHAPES = [(33, 47, 61), (64, 64, 64), (40, 36, 44), (9, 12, 7), (6, 6, 6), (512, 512, 512), (130, 70, 1026)]


def _bricks(gsz, div):
    return [D.mg_points(gsz, div, r) for r in range(div[0] * div[1] * div[2])]


# (every brick needs two points per direction)
OWN_CASES = [(g, d) for g in SHAPES for d in DIVS if all(gg >= 2 * dd for gg, dd in zip(g, d))]


@pytest.mark.parametrize("gsz,div", OWN_CASES, ids=[f"{'x'.join(map(str, g))}_{'x'.join(map(str, d))}" for g, d in OWN_CASES])
def test_ownership_partitions_every_level(gsz, div):
    """per direction the owned ranges tile every level; above G a brick's straddling children and parents lie on a direct neighbour"""
    bricks = _bricks(gsz, div)
    dims = D.mg_level_dims(gsz)
    G = D.mg_gather_level(gsz, div, gather_points=0)
    for lev, n in enumerate(dims):
        for a in range(3):
            # the bricks of one row along a, in order
            starts = sorted({h[a] for h, _ in bricks})
            ms = {h[a]: m[a] for h, m in bricks}
            rng = [D.mg_own(s, ms[s], lev) for s in starts]
            pos = 0
            for f, c in rng:
                assert f == pos and c >= 0
                pos += c
            assert pos == n[a], (lev, a, rng, n)
            if lev == 0 or lev > max(G, 1):
                continue
            # level lev's children (level lev - 1) and parents: first child owned, second child on the brick itself or on the + neighbour,
            # parent on the brick itself or on the - neighbour
            for q, (f, c) in enumerate(rng):
                ff, fc = D.mg_own(starts[q], ms[starts[q]], lev - 1)
                for I in range(f, f + c):
                    assert ff <= 2 * I < ff + fc
                    if 2 * I + 1 < dims[lev - 1][a]:
                        assert 2 * I + 1 <= ff + fc  # at most the + neighbour's first point
                        if 2 * I + 1 == ff + fc:
                            assert D.mg_own(starts[q + 1], ms[starts[q + 1]], lev - 1)[0] == 2 * I + 1
                for i in range(ff, ff + fc):
                    p = i >> 1
                    assert f - 1 <= p < f + c
                    if p == f - 1:
                        pf, pc = D.mg_own(starts[q - 1], ms[starts[q - 1]], lev)
                        assert pf <= p < pf + pc


def test_gather_level_rule():
    # 7 inner points along k in 3 bricks ([0, 2), [2, 5), [5, 7)): the last owns no point of level 2 -> G = 2 of 5 levels
    assert len(D.mg_level_dims((40, 40, 9))) == 5
    assert D.mg_own(5, 2, 2) == (2, 0)
    assert D.mg_gather_level((40, 40, 9), (1, 1, 3), gather_points=0) == 2
    # the size rule and its two ends
    assert D.mg_gather_level((130, 130, 130), (2, 2, 2)) == 2  # 64^3 > 32768 >= 32^3
    assert D.mg_gather_level((130, 130, 130), (2, 2, 2), gather_points=1 << 40) == 1
    assert D.mg_gather_level((130, 130, 130), (2, 2, 2), gather_points=0) == len(D.mg_level_dims((130,) * 3)) - 1
    assert D.mg_gather_level((6, 6, 6), (2, 1, 1)) == 0  # level 0 is the coarsest


# ---- the brick-wise cycle, restated
def _own_sl(h, m, lev):
    """slices (j, i, k) of a brick's owned points of level lev in the level's global array"""
    f = [D.mg_own(h[a], m[a], lev) for a in range(3)]
    return tuple(slice(f[a][0], f[a][0] + f[a][1]) for a in (1, 0, 2))


def _ghosted(glob, sl, fill=0.0):
    """the owned block plus one ghost layer, filled by slicing the level's global array (what the neighbours own; zero outside the box)"""
    P = np.pad(glob, 1, constant_values=fill)
    return P[tuple(slice(s.start, s.stop + 2) for s in sl)].copy()


def _ss_p(Up, W):
    wx, wy, wz, _ = W
    ip, im = Up[1:-1, 2:, 1:-1], Up[1:-1, :-2, 1:-1]
    jp, jm = Up[2:, 1:-1, 1:-1], Up[:-2, 1:-1, 1:-1]
    kp, km = Up[1:-1, 1:-1, 2:], Up[1:-1, 1:-1, :-2]
    return wx * ip + wx * im + wy * jp + wy * jm + wz * kp + wz * km


class Bricks:
    def __init__(self, gsz, div, omg, G):
        self.bricks = _bricks(gsz, div)
        self.n0 = tuple(v - 2 for v in gsz)
        self.dims = D.mg_level_dims(gsz)
        self.omg, self.G = omg, G

    def _w(self, lev, sl, R):
        return tuple(w[sl] for w in M.weights(self.n0, lev, R))

    def assemble(self, blocks, lev, R, fill=0.0):
        ni, nj, nk = self.dims[lev]
        out = np.full((nj, ni, nk), fill, dtype=R)
        for (h, m), blk in zip(self.bricks, blocks):
            out[_own_sl(h, m, lev)] = blk
        return out

    def smooth(self, xs, bs, lev):
        """one sweep on every brick; the input's ghosts by a face exchange (slicing)"""
        R = bs[0].dtype.type
        glob = None if xs is None else self.assemble(xs, lev, R)
        out = []
        for q, (h, m) in enumerate(self.bricks):
            sl = _own_sl(h, m, lev)
            W = self._w(lev, sl, R)
            b = bs[q]
            if glob is None:
                Up = np.zeros(tuple(s.stop - s.start + 2 for s in sl), dtype=R)
            else:
                Up = _ghosted(glob, sl)
            u = Up[1:-1, 1:-1, 1:-1]
            out.append(u + ((_ss_p(Up, W) - b) / W[3] - u) * R(self.omg))
        return out

    def restrict(self, xs, bs, lev):
        """b_{lev+1} per brick: the owned children's residual computed by the brick, the + neighbours' first layer taken from what they
        computed (everything else of the exchanged array NaN: a read of it would show)"""
        R = bs[0].dtype.type
        xg = self.assemble(xs, lev, R)
        res = []
        for q, (h, m) in enumerate(self.bricks):
            sl = _own_sl(h, m, lev)
            W = self._w(lev, sl, R)
            Up = _ghosted(xg, sl)
            res.append(bs[q] - (_ss_p(Up, W) - W[3] * Up[1:-1, 1:-1, 1:-1]))
        # the first owned layer on the - faces, as the neighbours compute and send it
        first = []
        for r_, (h, m) in zip(res, self.bricks):
            f = np.full_like(r_, np.nan)
            f[0, :, :], f[:, 0, :], f[:, :, 0] = r_[0, :, :], r_[:, 0, :], r_[:, :, 0]
            first.append(f)
        firstg = self.assemble(first, lev, R, fill=np.nan)
        out = []
        for q, (h, m) in enumerate(self.bricks):
            sl = _own_sl(h, m, lev)
            cs = _own_sl(h, m, lev + 1)
            ext = _ghosted(firstg, sl, fill=np.nan)[1:, 1:, 1:]  # owned + the + ghost layer
            ext[:-1, :-1, :-1] = res[q]
            n = self.dims[lev]
            lo = [2 * c.start - s.start for c, s in zip(cs, sl)]
            hi = [min(2 * c.stop, nn) - s.start for c, s, nn in zip(cs, sl, (n[1], n[0], n[2]))]
            kids = ext[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
            out.append(M._pair(M._pair(M._pair(kids, 2), 1), 0))
        return out

    def prolong(self, xs, xcg, lev):
        """u = x + R(1.8 x_c(parent)) with the parents from the coarse level's global array (a ghost on the - side, or the gathered copy)"""
        R = xs[0].dtype.type
        out = []
        for q, (h, m) in enumerate(self.bricks):
            sl = _own_sl(h, m, lev)
            cs = _own_sl(h, m, lev + 1)
            Cp = _ghosted(xcg, cs, fill=np.nan)  # coarse owned + one ghost layer
            idx = [np.arange(s.start, s.stop) // 2 - (c.start - 1) for s, c in zip(sl, cs)]
            par = Cp[np.ix_(idx[0], idx[1], idx[2])]
            out.append(xs[q] + R(M.ALPHA) * par)
        return out

    def cycle(self, bs, lev):
        if lev == len(self.dims) - 1:
            xs = self.smooth(None, bs, lev)
            for _ in range(7):
                xs = self.smooth(xs, bs, lev)
            return xs
        xs = self.smooth(self.smooth(None, bs, lev), bs, lev)
        bc = self.restrict(xs, bs, lev)
        R = bs[0].dtype.type
        if lev + 1 < self.G:
            xcg = self.assemble(self.cycle(bc, lev + 1), lev + 1, R)
        else:  # the gathered levels: every rank runs the single-domain cycle on the all-gathered b
            xcg = M.vcycle(self.assemble(bc, lev + 1, R), lev + 1, self.n0, self.omg)
        u = self.prolong(xs, xcg, lev)
        return self.smooth(self.smooth(u, bs, lev), bs, lev)


BRICK_CASES = [((33, 47, 61), (2, 2, 2)), ((33, 47, 61), (3, 1, 2)), ((34, 30, 40), (1, 3, 1)), ((40, 40, 9), (1, 1, 3)),
               ((64, 64, 64), (2, 1, 2)), ((6, 6, 6), (2, 1, 1)), ((20, 21, 22), (2, 2, 2))]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("gsz,div", BRICK_CASES, ids=[f"{'x'.join(map(str, g))}_{'x'.join(map(str, d))}" for g, d in BRICK_CASES])
def test_brickwise_cycle_equals_single_domain(gsz, div, prec):
    """every allowed G, the brick-wise cycle assembled = mg_parity.vcycle, bit for bit"""
    R = np.float32 if prec == "f32" else np.float64
    n0 = tuple(v - 2 for v in gsz)
    rng = np.random.default_rng(5)
    b = rng.standard_normal((n0[1], n0[0], n0[2])).astype(R)
    ref = M.vcycle(b, 0, n0, 0.8)
    dims = D.mg_level_dims(gsz)
    Gmax = D.mg_gather_level(gsz, div, gather_points=0)
    for G in sorted({g for g in range(1, Gmax + 1)} | {Gmax}):
        if len(dims) == 1:
            G = 0
        B = Bricks(gsz, div, 0.8, G)
        bs = [b[_own_sl(h, m, 0)] for h, m in B.bricks]
        got = B.assemble(B.cycle(bs, 0), 0, R)
        assert got.tobytes() == ref.tobytes(), f"G = {G}: the brick-wise cycle differs"


def test_early_gather_case_is_covered():
    """one of the cases above has a brick without a point of a level above the coarsest"""
    hits = []
    for gsz, div in BRICK_CASES:
        dims = D.mg_level_dims(gsz)
        for lev in range(1, len(dims) - 1):
            if any(D.mg_own(h[a], m[a], lev)[1] < 1 for h, m in _bricks(gsz, div) for a in range(3)):
                hits.append((gsz, div, lev))
    assert hits


def test_ownership_of_all_divisions_small():
    """exhaustive on small extents: ranges partition [0, ceil(n / 2^l)) for every split of n into bricks of >= 2 points"""
    for n in range(2, 40):
        for parts in range(1, n // 2 + 1):
            base, rem = divmod(n, parts)
            heads = list(itertools.accumulate([0] + [base + (r < rem) for r in range(parts)]))
            for lev in range(7):
                pos = 0
                for r in range(parts):
                    f, c = D.mg_own(heads[r], heads[r + 1] - heads[r], lev)
                    assert f == pos and c >= 0
                    pos += c
                assert pos == -(-n // (1 << lev))
