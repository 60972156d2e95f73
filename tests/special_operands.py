"""Operand families that reach the special branches of the hoisted division inside a pass (importable without a GPU).

`fastdiv` / `mediumdiv` (cubez_amd/csrc/cz_k_fastdiv.h) replace n / d by products with reciprocals made once per launch and pick one of two
by the class V_DIV_SCALE puts the numerator in.  czhip_selftest_fastdiv proves the function for every numerator; whether a PASS that inlines
it hands such numerators on unharmed -- through LDS, DPP, packed or flushing operations, every fused stage -- shows only on fields that
produce them in every stage.  Ordinary values (uniform(-1, 1)) never do.  Four families, all finite, random signs (FP32 / FP64):

    sub    +-0 (one value in sixteen), the smallest subnormal, random subnormals
    tiny   the above (three values in ten) and normals with exponent -125 .. -101 / -1021 .. -967, most of them from the lower middle of
           that range, where a value alone and a sum of seven are both tiny numerators
    mixed  zeros, subnormals, normals with exponent -120 .. -101 / -1016 .. -967 and uniform(0, 1): the family of
           tests/test_gpu_jac3_steps.py::test_update_on_zeros_subnormals_and_tiny_values (FP32: `special`, moved here unchanged)
    huge   on the lattice j % 3 == i % 3 == k % 3 == 1 of the padded array (no 7-point stencil sees two of its cells) every other cell
           (a checkerboard in j and i) holds 2^99 .. 2^119 / 2^775 .. 2^999; all other cells hold zeros, tiny and ordinary values

The classes of a numerator n = ss - b with divisor d, after the CDNA ISA manual's description of V_DIV_SCALE_F32 / _F64 (S2 = n, S1 = d):
    zero                n == 0
    quotient subnormal  |n / d| < 2^emin                          ("S2 / S1 is DENORM")
    tiny                biased exponent(n) <= 23 / 53, i.e. |n| < 2^-103 / 2^-969   ("numerator is tiny")
    huge                exponent(n) - exponent(d) >= 96 / 768     ("N / D near MAX_FLOAT")
    ordinary            everything else
What the instruction does with them on gfx950 (measured, profiles/r21/div_scale_classes.txt; d = 6 and 6.2): quotient-subnormal AND tiny
numerators get the NUMERATOR scaled by 2^64 / 2^128 with VCC set, the denominator comes back as d -- `fastdiv` keeps r1 and div_fmas scales
the quotient back down, rounding once into the subnormal range; only huge numerators get the DENOMINATOR scaled, and they alone select r1s.
So `huge` is the family that tells the two reciprocals apart, `sub` and `tiny` the ones that tell a flushing or twice-rounding operation.
The classes serve the counting of tests/test_special_operands.py only; correctness on the GPU is always bit parity with the oracle's sweeps.
"""
from __future__ import annotations

import numpy as np

FAMILIES = ("sub", "tiny", "mixed", "huge")
CLASSES = ("zero", "qsub", "tiny", "huge", "ordinary")
# per precision: uint view, mantissa bits, emin, tiny-normal exponents [lo, hi), mixed's tiny exponents, huge exponents [lo, hi], the tiny / huge rules
FMT = {
    "f32": dict(R=np.float32, U=np.uint32, mant=23, emin=-126, tiny=(-125, -100), mixed=(-120, -100), huge=(99, 119), tiny_below=-103, huge_gap=96),
    "f64": dict(R=np.float64, U=np.uint64, mant=52, emin=-1022, tiny=(-1021, -966), mixed=(-1016, -966), huge=(775, 999), tiny_below=-969, huge_gap=768),
}
BOXES = [(12, 10, 60), (11, 9, 61)]  # rows of 64 and 65 elements
# the share of the family's class among the inner points that every stage of every compared pass must reach (conditions on the inputs)
FLOORS = {"sub": ("qsub", 0.90), "tiny": ("tiny", 0.50), "huge": ("huge", 0.10)}
MIXED_FLOOR = 0.02  # tiny + quotient-subnormal, stage 1 only


def special(rng, shape):
    """per element one of: 0, -0, the smallest subnormal, a random subnormal, a value in [2^-120, 2^-100], an ordinary value; random signs"""
    kind = rng.integers(0, 6, shape)
    sub = rng.integers(1, 1 << 23, shape).astype(np.uint32).view(np.float32)
    tiny = np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(-120, -100, shape)).astype(np.float32)  # exponents -120 .. -101
    mag = np.select([kind <= 1, kind == 2, kind == 3, kind == 4], [np.float32(0), np.float32(2.0 ** -149), sub, tiny],
                    rng.uniform(0.0, 1.0, shape).astype(np.float32)).astype(np.float32)
    x = np.copysign(mag, rng.choice(np.array([-1.0, 1.0], dtype=np.float32), shape)).astype(np.float32)
    assert np.isfinite(x).all()
    return x


def _parts(rng, shape, prec, exps, peaked=False):
    f = FMT[prec]
    R = f["R"]
    minsub = np.ldexp(1.0, f["emin"] - f["mant"])
    sub = rng.integers(1, 1 << f["mant"], shape, dtype=np.int64).astype(f["U"]).view(R)
    # exponents over the whole range, the low ones more often (u^2): a numerator is a sum of seven values and takes the largest one's exponent
    e = exps[0] + np.floor((exps[1] - exps[0]) * rng.uniform(0.0, 1.0, shape) ** 2).astype(np.int64)
    if peaked:
        # nine in ten from lo + 2 .. hi - 5 (the low ones more often), where a value alone is a tiny numerator with a normal quotient (the
        # pass from zero divides -b) and a sum of seven stays tiny; one in ten from the whole range
        lo, hi = exps[0] + 2, exps[1] - 4
        main = lo + np.floor((hi - lo) * rng.uniform(0.0, 1.0, shape) ** 2).astype(np.int64)
        e = np.where(rng.integers(0, 10, shape) > 0, main, rng.integers(exps[0], exps[1], shape))
    tiny = np.ldexp(rng.uniform(1.0, 2.0, shape), e).astype(R)
    return R(0), R(minsub), sub, tiny


def _signed(rng, mag, R):
    x = np.copysign(mag, rng.choice(np.array([-1.0, 1.0]), mag.shape)).astype(R)
    assert np.isfinite(x).all() and x.dtype == R
    return x


def family(name, rng, shape, prec, dense=False):
    """one field of the family on a padded array [j, i, k].  dense (huge only): one cell in six, at random, holds a huge value instead of half
    the lattice -- for the operands of a pass that starts from zero, whose first stage divides -b and sees no neighbour"""
    f = FMT[prec]
    R = f["R"]
    if name == "mixed" and prec == "f32":
        return special(rng, shape)
    zero, minsub, sub, tiny = _parts(rng, shape, prec, f["mixed"] if name == "mixed" else f["tiny"], peaked=name != "mixed")
    ordinary = rng.uniform(0.0, 1.0, shape).astype(R)
    if name == "sub":
        kind = rng.integers(0, 16, shape)  # (one zero in sixteen: a zero numerator is in no class)
        mag = np.select([kind == 0, kind <= 3], [zero, minsub], sub)
    elif name == "tiny":
        kind = rng.integers(0, 10, shape)
        mag = np.select([kind == 0, kind == 1, kind == 2], [zero, minsub, sub], tiny)
    elif name == "mixed":
        kind = rng.integers(0, 6, shape)
        mag = np.select([kind <= 1, kind == 2, kind == 3, kind == 4], [zero, minsub, sub, tiny], ordinary)
    elif name == "huge":
        kind = rng.integers(0, 3, shape)
        mag = np.select([kind == 0, kind == 1], [zero, tiny], ordinary).astype(R)
        j, i, k = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
        lattice = (j % 3 == 1) & (i % 3 == 1) & (k % 3 == 1)
        big = np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(f["huge"][0], f["huge"][1] + 1, shape)).astype(R)
        # half the lattice: every other cell of it (a checkerboard, its phase drawn), so that the share does not hang on the draw
        half = lattice & ((j // 3 + i // 3) % 2 == rng.integers(0, 2))  # (not k: with it the half would be one red-black colour)
        mag = np.where((rng.integers(0, 6, shape) == 0) if dense else half, big, mag)
    else:
        raise ValueError(name)
    return _signed(rng, mag.astype(R), R)


def fields(name, prec, shape, seed=5):
    """(p, b) of the family, seeded"""
    rng = np.random.default_rng(seed)
    return family(name, rng, shape, prec), family(name, rng, shape, prec)


# the pass from zero (czhip_jacobi2_from_zero_made_async): the start vector is a literal zero, the right-hand side is read (op 0) or made on the
# way from three operands (op 1: a x + y, blas_triad; op 2: x + a (z - bb y), blas_bicg_1) and stored
ZERO_A, ZERO_BB = {0: 0.0, 1: -0.7, 2: 0.6}, 1.3


def zero_pass_operands(name, prec, shape, seed=5):
    """(x, y, z) of the family (huge: dense); op 0 reads z as the right-hand side"""
    rng = np.random.default_rng(100 + seed)
    return tuple(family(name, rng, shape, prec, dense=True) for _ in range(3))


def zero_pass_rhs(ko, op, x, y, z, sz, idx):
    """the right-hand side the pass makes, by the oracle's own vector kernels: outside the inner box it keeps z's values"""
    b = z.copy()
    if op == 1:
        ko.blas_triad(b, x, y, ZERO_A[1], sz, idx)
    elif op == 2:
        ko.blas_bicg_1(b, x, y, ZERO_A[2], ZERO_BB, sz, idx)
    assert np.isfinite(b).all()
    return b


def classify(n, d, prec):
    """the class index (into CLASSES) of every numerator n for the divisor d (a scalar or an array like n)"""
    f = FMT[prec]
    n = np.asarray(n)
    a = np.abs(n).astype(np.longdouble)
    dl = np.abs(np.asarray(d)).astype(np.longdouble)
    en = np.frexp(np.abs(n).astype(np.float64))[1] - 1  # (floor(log2 |n|); a subnormal's is below emin, as the rule wants)
    ed = np.frexp(np.abs(np.asarray(d)).astype(np.float64))[1] - 1
    out = np.full(n.shape, CLASSES.index("ordinary"))
    out[(en - ed) >= f["huge_gap"]] = CLASSES.index("huge")
    out[a < np.ldexp(np.longdouble(1), f["tiny_below"])] = CLASSES.index("tiny")
    out[a < dl * np.ldexp(np.longdouble(1), f["emin"])] = CLASSES.index("qsub")
    out[n == 0] = CLASSES.index("zero")
    return out


def shares(cls):
    """{class name: share of the points}"""
    return {c: float((cls == i).mean()) for i, c in enumerate(CLASSES)}


# ---- the oracle's sweeps with the numerators of every stage
def inner(sz, idx, g=2):
    ist, ied, jst, jed, kst, ked = idx
    return slice(jst + g - 1, jed + g), slice(ist + g - 1, ied + g), slice(kst + g - 1, ked + g)


def numerators(p, b, sz, idx, cf):
    """n = ss - b at the inner points, with the oracle's operations in its order (REAL, one rounding each)"""
    js, is_, ks = inner(sz, idx)
    sh = lambda dj, di, dk: p[js.start + dj:js.stop + dj, is_.start + di:is_.stop + di, ks.start + dk:ks.stop + dk]  # noqa: E731
    c = [cf.dtype.type(v) for v in cf]
    ss = c[0] * sh(0, 1, 0) + c[1] * sh(0, -1, 0) + c[2] * sh(1, 0, 0) + c[3] * sh(-1, 0, 0) + c[4] * sh(0, 0, 1) + c[5] * sh(0, 0, -1)
    n = ss - b[js, is_, ks]
    assert n.dtype == p.dtype
    return n


def colour_mask(sz, idx, ofst, colour):
    """the inner points psor2sma_core updates: k = kst + mod(i + j + ofst + colour, 2), ked, 2 (Fortran indices)"""
    ist, ied, jst, jed, kst, ked = idx
    j, i, k = np.meshgrid(np.arange(jst, jed + 1), np.arange(ist, ied + 1), np.arange(kst, ked + 1), indexing="ij")
    return (k - kst) % 2 == (i + j + ofst + colour) % 2


def jacobi_sweeps(ko, p, b, sz, idx, cf, omg, n, idx_first=None):
    """n oracle Jacobi sweeps from p: (final field, [wide residual of each], [numerators of each stage]); every sweep's field is checked
    finite (condition (a) of tests/test_special_operands.py).  idx_first: the box of the first sweep where it is larger than idx (the pass
    of a decomposed brick makes its first sweep one layer into the ghost cells of its neighbours)"""
    a, w, res, nums = p.copy(), np.zeros_like(p), [], []
    for s in range(n):
        box = idx_first if (s == 0 and idx_first is not None) else idx
        nums.append(numerators(a, b, sz, box, cf))
        wide = np.zeros(1)
        ko.jacobi(a, sz, box, cf, omg, b, w, wide=wide)
        assert np.isfinite(a).all(), f"sweep {s + 1}: a field that is not finite"
        res.append(float(wide[0]))
    return a, res, nums


def colour_sweeps(ko, p, b, sz, idx, cf, omg, ofst, iterations, idx_first=None):
    """`iterations` red-black iterations (colour 0 then 1): (final field, [wide residual of each ITERATION], [numerators of each colour sweep
    at the points it updates]); every sweep's field is checked finite.  idx_first: the box of the very first colour sweep (see jacobi_sweeps)"""
    a, res, nums = p.copy(), [], []
    for it in range(iterations):
        wide = np.zeros(1)
        for colour in (0, 1):
            box = idx_first if (it == 0 and colour == 0 and idx_first is not None) else idx
            nums.append(numerators(a, b, sz, box, cf)[colour_mask(sz, box, ofst, colour)])
            ko.psor2sma_core(a, sz, box, cf, ofst, colour, omg, b, wide=wide)
            assert np.isfinite(a).all(), f"iteration {it + 1} colour {colour}: a field that is not finite"
        res.append(float(wide[0]))
    return a, res, nums


def coef(R, unit, seed=0):
    if unit:
        return np.array([1, 1, 1, 1, 1, 1, 6], dtype=R)
    cf = np.random.default_rng(900 + seed).uniform(0.5, 1.5, 7).astype(R)
    cf[6] = 6.2
    return cf
