"""The conditions tests/test_gpu_special_operands.py rests on, checked on the oracle alone (CPU): for every family, precision
and pass compared on the GPU, every field of every sweep is finite, every STAGE of the pass meets the family's class of numerators in the
share tests/special_operands.py FLOORS asks for, and the oracle's residual sums are what the GPU test then demands (0.0 for sub and tiny,
+inf for huge).  These are conditions on the inputs, not tolerances: a case that misses one needs another generator."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import special_operands as S  # noqa: E402
from oracle import cz_oracle as O  # noqa: E402

OMG_J, OMG_RB = 0.9, 1.3
# pass -> (its sweeps, stages); the single sweeps of stencil_k are stage 1 of these
PASSES = {"jacobi2_unit": 2, "jacobi2_coef": 2, "jacobi3_unit": 3, "jacobi3_coef": 3, "rb_ofst0": 4, "rb_ofst1": 4, "rb_coef_ofst0": 4, "rb_coef_ofst1": 4,
          # the shell-slab pass of a decomposed brick (box 12x10x60 only): first sweep / colour one layer into the ghost cells of X+ and Z+
          "split_jacobi2_unit": 2, "split_jacobi2_coef": 2, "split_rb2_ofst0": 2, "split_rb2_coef_ofst1": 2}
# the pass from a literal zero, right-hand side read (op 0) or made (ops 1, 2): its first stage divides -b
PASSES.update({f"zero{op}_jacobi2_unit": 2 for op in (0, 1, 2)})
PASSES.update({f"zero{op}_rb2_coef_ofst{o}": 2 for op in (0, 1, 2) for o in (0, 1)})
SPLIT_PATTERN = [0, 1, 0, 0, 0, 1]


def split_boxes(box):
    """(idx, idx1) of tests/test_gpu_special_operands.py::test_shell_slabs_and_interior"""
    n = [box[0], box[0], box[1], box[1], box[2], box[2]]
    idx = [(1 if v else 2) if f % 2 == 0 else (n[f] if v else n[f] - 1) for f, v in enumerate(SPLIT_PATTERN)]
    return idx, [idx[f] + ((1 if f % 2 else -1) if v else 0) for f, v in enumerate(SPLIT_PATTERN)]


family_of = [None]  # the family of the case in hand (the pass from zero draws its own operands from it)


def run_pass(name, ko, p, b, sz, idx):
    """(final field, residuals, numerators per stage, divisor)"""
    R = ko.real
    unit = "coef" not in name
    cf = S.coef(R, unit)
    if name.startswith("zero"):
        x, y, z = S.zero_pass_operands(family_of[0], "f32" if R == np.float32 else "f64", p.shape)
        b = S.zero_pass_rhs(ko, int(name[4]), x, y, z, sz, idx)
        p = np.zeros_like(p)
        if "jacobi" in name:
            return S.jacobi_sweeps(ko, p, b, sz, idx, cf, OMG_J, 2) + (cf[6],)
        return S.colour_sweeps(ko, p, b, sz, idx, cf, OMG_RB, int(name[-1]), 1) + (cf[6],)
    if name.startswith("split"):
        idx, idx1 = split_boxes(sz)
        if "jacobi" in name:
            return S.jacobi_sweeps(ko, p, b, sz, idx, cf, OMG_J, 2, idx_first=idx1) + (cf[6],)
        return S.colour_sweeps(ko, p, b, sz, idx, cf, OMG_RB, int(name[-1]), 1, idx_first=idx1) + (cf[6],)
    if name.startswith("jacobi"):
        return S.jacobi_sweeps(ko, p, b, sz, idx, cf, OMG_J, PASSES[name]) + (cf[6],)
    return S.colour_sweeps(ko, p, b, sz, idx, cf, OMG_RB, int(name[-1]), 2) + (cf[6],)


def _case(family, prec, box):
    ni, nj, nk = box
    sz, idx = [ni, nj, nk], [2, ni - 1, 2, nj - 1, 2, nk - 1]
    p, b = S.fields(family, prec, (nj + 4, ni + 4, nk + 4))
    return sz, idx, p, b


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_the_numerators_are_the_oracles(prec):
    """p + ((n / dd) - p) * omg with n from special_operands.numerators is the oracle's sweep bit for bit, on every family: the classes are
    counted on the numerators the oracle divides"""
    ko = O.Kernels("oracle", prec)
    R = ko.real
    for family in S.FAMILIES:
        sz, idx, p, b = _case(family, prec, S.BOXES[1])
        for unit in (1, 0):
            cf = S.coef(R, unit)
            a, _, nums = S.jacobi_sweeps(ko, p, b, sz, idx, cf, OMG_J, 1)
            ins = S.inner(sz, idx)
            with np.errstate(all="ignore"):
                want = p[ins] + ((nums[0] / cf[6]) - p[ins]) * R(OMG_J)
            assert want.dtype == R and a[ins].tobytes() == want.tobytes(), (family, prec, unit)
            rb, _, nrb = S.colour_sweeps(ko, p, b, sz, idx, cf, OMG_RB, 1, 1)
            m = S.colour_mask(sz, idx, 1, 0)
            with np.errstate(all="ignore"):
                want = p[ins][m] + ((nrb[0] / cf[6]) - p[ins][m]) * R(OMG_RB)
            first = p.copy()
            ko.psor2sma_core(first, sz, idx, cf, 1, 0, OMG_RB, b, wide=np.zeros(1))
            assert first[ins][m].tobytes() == want.tobytes() and first[ins][~m].tobytes() == p[ins][~m].tobytes(), (family, prec, unit)


def test_the_classifier_on_the_boundaries():
    for prec, d in (("f32", np.float32(6)), ("f64", np.float64(6.2))):
        f = S.FMT[prec]
        R = f["R"]
        two = lambda e: R(np.ldexp(1.0, e))  # noqa: E731
        below = lambda x: np.nextafter(x, R(0))  # noqa: E731
        ed = math.frexp(float(d))[1] - 1
        n = np.array([0.0, -0.0, two(f["emin"] - f["mant"]), below(two(f["tiny_below"])), two(f["tiny_below"]), R(1),
                      below(two(f["huge_gap"] + ed)), two(f["huge_gap"] + ed), -two(f["huge_gap"] + ed + 3)], dtype=R)
        got = [S.CLASSES[c] for c in S.classify(n, d, prec)]
        assert got == ["zero", "zero", "qsub", "tiny", "ordinary", "ordinary", "ordinary", "huge", "huge"], (prec, got)
        # the quotient's own boundary: d * 2^emin is the first numerator whose quotient is normal
        edge = (np.longdouble(d) * np.ldexp(np.longdouble(1), f["emin"])).astype(R)
        got = [S.CLASSES[c] for c in S.classify(np.array([below(edge), np.nextafter(edge, R(1))], dtype=R), d, prec)]
        assert got == ["qsub", "tiny"], (prec, got)


@pytest.mark.parametrize("name", list(PASSES))
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("family", S.FAMILIES)
def test_every_stage_meets_the_family(family, prec, name):
    ko = O.Kernels("oracle", prec)
    for box in (S.BOXES[:1] if name.startswith("split") else S.BOXES):
        sz, idx, p, b = _case(family, prec, box)
        family_of[0] = family
        a, res, nums, dd = run_pass(name, ko, p, b, sz, idx)
        # (a) finiteness: special_operands.jacobi_sweeps / colour_sweeps assert it on the field of every sweep; here the inputs and numerators
        assert np.isfinite(p).all() and np.isfinite(b).all() and np.isfinite(a).all() and all(np.isfinite(n).all() for n in nums), (family, prec, name, box)
        # (b) the share of the family's class in every stage
        per_stage = [S.shares(S.classify(n, dd, prec)) for n in nums]
        for s, sh in enumerate(per_stage, 1):
            print(f"{family} {prec} {name} {'x'.join(map(str, box))} stage {s}: " + "  ".join(f"{c} {v:.3f}" for c, v in sh.items()))
        if family == "mixed":
            first = per_stage[0]["tiny"] + per_stage[0]["qsub"]
            assert first >= S.MIXED_FLOOR, (family, prec, name, box, first)
            print(f"mixed {prec} {name}: tiny + quotient-subnormal after stage 1: {[sh['tiny'] + sh['qsub'] for sh in per_stage[1:]]}")
        else:
            cls, floor = S.FLOORS[family]
            assert all(sh[cls] >= floor for sh in per_stage), (family, prec, name, box, [sh[cls] for sh in per_stage])
        # the residuals the oracle returns
        if family in ("sub", "tiny"):
            assert all(r == 0.0 for r in res), (family, prec, name, box, res)
        elif family == "huge":
            assert all(r == math.inf for r in res), (family, prec, name, box, res)
        else:
            assert all(math.isfinite(r) and r > 0.0 for r in res), (family, prec, name, box, res)
