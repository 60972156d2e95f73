"""Random call sequences on one handle against a fresh twin (-m gpu): the walks of tests/walk_plan.py.

The walked handle makes a walk's 24 calls in order.  At an observed step the test records the step's return value, the whole padded field()
and what belongs to the kind of step (solve / sweeps: iter, history(), the counters and flags of info(); get_residual: the bytes written and
sumsq; sub_grad: the three velocity base arrays entire, sentinels included; precondition: z; closed_mean: the float); after an unobserved
step it reads nothing and does not synchronise.  For every observed step a twin is made from the documented state alone: set-up with the
same arguments, the RHS sub-history replayed, eps and itr_max set, set_field with the brick of the field recorded at the last observed step,
then the calls since, with the same carriers and streams.  Everything recorded must be equal: bytes, `==` on floats and on info() entries,
no tolerance -- both sides are this library on this GPU, and its sums are ordered.  (info()["field_form"] names the last field call, which
in a twin may be the twin's own set_field: it is compared where the calls since the last observed step hold a field call.)

Default mode: the walk first, the twins after the walked handle is closed.  One walk per group also runs with its twin alive beside it,
call by call (two handles on one context).

Group C: the ranks of a division as threads of the local world (test_gpu_neumann._ranks); every rank walks its own handle on its brick
of the seeded global arrays and makes its own twins, all of them collectively, and nothing is asserted on a rank thread -- a rank that
stopped would leave its peers in a collective -- but after the threads have ended.  Of a rank's padded field the layers beyond a cut side
are left out: they are copies of the neighbour's cells, which its own rank compares, refreshed by the exchange of whatever call wrote
the field last (DESIGN.md §5.17 lists them with the caches).  The last solve is gathered and compared as the family's decomposed tests do.

The twins are this library too, so two ties to the independent restatements: the last solve of every walk is compared with the restatement
run from the seeded right-hand side, the state and the recorded field, by the helper and under the bar of the family's own GPU test
(test_gpu_problem._compare; test_gpu_neumann._close, FP32 after periodic_parity.premise_f32); and every observed closed_mean(0) with the
restated mean of the seeded right-hand side under closed_parity.mean_tol, the bar of tests/test_gpu_project.py -- a mean both sides get
wrong alike would stay equal.  walk_plan.tail_length says why the FP64 pcg walks end outside the closed mode on a seeded field: at
(33, 47, 61) in the triply periodic box the FP64 answer of a walk's own field differed from the restatement by 1 ulp of the unshifted
iterate (1.1e-16) in a cell that the shift by the mean had brought to 1.5e-5, where E was 0 and 8 ulp of the cell is 1.4e-20
(|d| / bound = 8192; 474 of 122 655 cells beyond the bound, history equal to 14 digits, twin equal bit for bit)."""
import contextlib
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closed_parity as CB  # noqa: E402
import periodic_parity as P  # noqa: E402
import problem_parity as PP  # noqa: E402
import project_parity as J  # noqa: E402
import test_gpu_neumann as TN  # noqa: E402
import test_gpu_problem as TP  # noqa: E402
import walk_plan as W  # noqa: E402

pytestmark = pytest.mark.gpu
OUTSIDE = -77.0  # elements of a base array outside the brick
SOLVE_INFO = ("bicg_fused", "rb4_passes", "exact_reruns", "cg_fused", "jac3_passes", "mg_cycles", "mg_exchanges", "lagged_reduce", "neumann", "closed",
              "periodic", "pass_kind", "buffers")
FIELD_CALLS = ("set_rhs", "set_field", "get_residual", "add_field", "set_rhs_div", "sub_grad")


class _Ctx:
    """torch, one side stream and some work to put in front of an import on it; the tensors handed to the library stay alive to the end"""

    def __init__(self):
        self.torch = TP._torch()
        self.side = self.torch.cuda.Stream()
        self.junk = self.torch.empty(64 * 1024 * 1024 // 8, dtype=self.torch.float64, device="cuda")
        self.keep = []
        self.torch.cuda.synchronize()

    def on(self, carrier):
        return self.torch.cuda.stream(self.side) if carrier == "device_side" else contextlib.nullcontext()

    def tensor(self, a, carrier):
        """a on the device: on torch's current stream, or (inside `on`) on the side stream behind fills of a large array and of the tensor"""
        t = self.torch
        if carrier == "device":
            x = t.from_numpy(np.ascontiguousarray(a)).cuda()
        else:
            h = t.from_numpy(np.ascontiguousarray(a)).pin_memory()
            x = t.empty(a.shape, dtype=h.dtype, device="cuda")
            for _ in range(4):
                self.junk.fill_(1.0)
            x.fill_(123.0)
            x.copy_(h, non_blocking=True)
            self.keep.append(h)
        self.keep.append(x)
        return x


def _based(a, off, pad):
    """(base, view): a inside a sentinel-filled numpy base, at offset `off`, `pad` more elements per direction"""
    base = np.full(tuple(n + q for n, q in zip(a.shape, pad)), OUTSIDE, dtype=a.dtype)
    view = base[tuple(slice(o, o + n) for o, n in zip(off, a.shape))]
    view[...] = a
    return base, view


def _sub(base, off, shape):
    return base[tuple(slice(o, o + n) for o, n in zip(off, shape))]


def _carried(ctx, a, carrier):
    """the array as its carrier hands it over (device carriers: call inside ctx.on(carrier))"""
    if carrier == "c_order":
        return np.ascontiguousarray(a)
    if carrier == "fortran":
        return np.asfortranarray(a)
    if carrier == "slice":  # (test_gpu_problem._layouts' slice: rows that start anywhere)
        return _based(a, (2, 1, 3), (3, 2, 5))[1]
    return ctx.tensor(a, carrier)


def _host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _new(c):
    from cubez_amd import CZ
    cz = CZ(c["prec"], quiet=True)
    assert cz.setup(PP.args(c, c.get("div"))) == 1
    return cz


def _part(cz, c, a):
    """this rank's brick of an array of the whole domain [i, j, k]"""
    return a[cz.global_slice()] if "div" in c else a


def _field(cz, c):
    """the padded field; of a decomposed handle without the layers beyond a cut side (the neighbour's cells)"""
    f = cz.field()
    if "div" in c:
        loc = cz.local()
        for d, ax in enumerate((1, 0, 2)):  # the array axis [j, i, k] of direction X, Y, Z
            sl = [slice(None)] * 3
            if loc["head"][d] > 1:
                sl[ax] = slice(0, PP.G)
                f[tuple(sl)] = 0
            if loc["head"][d] - 1 + loc["size"][d] < c["gsz"][d]:
                sl[ax] = slice(-PP.G, None)
                f[tuple(sl)] = 0
    return f


def _call(ctx, cz, c, st, state, observe, field_call_since):
    """one step on one handle; the record where observed"""
    k = st["kind"]
    rec, ret = {}, None
    gsz = tuple(cz.local()["size"]) if "div" in c else tuple(c["gsz"])
    if k == "state":
        for name, arg in st["calls"]:
            getattr(cz, name)(arg)
    elif k in ("set_rhs", "set_field"):
        a = _part(cz, c, (W.rhs_data if k == "set_rhs" else W.field_data)(c, st["seed"]))
        with ctx.on(st["carrier"]):
            x = _carried(ctx, a, st["carrier"])
            getattr(cz, k)(x)
            if st["carrier"] == "device_side":
                x.zero_()  # (the caller may reuse its array at once)
    elif k == "set_rhs_div":
        vel = W.velocity_data(c, st["seed"], state)
        with ctx.on(st["carrier"]):
            if st["carrier"] == "slice":
                xs = [_based(a, (1, 2, 3), (2, 3, 5))[1] for a in vel]
            else:
                xs = [_carried(ctx, a, st["carrier"]) for a in vel]
            ret = cz.set_rhs_div(*xs, scale=st["scale"], want_norm=observe)
    elif k == "sub_grad":
        vel = W.velocity_data(c, st["seed"], state)
        bases = [_based(a, (1, 2, 3), (2, 3, 5))[0] for a in vel]
        with ctx.on(st["carrier"]):
            if st["carrier"] != "slice":
                bases = [ctx.tensor(b, st["carrier"]) for b in bases]
            cz.sub_grad(*[_sub(b, (1, 2, 3), gsz) for b in bases], scale=st["scale"])
            if observe:
                rec["velocity"] = [_host(b).tobytes() for b in bases]
    elif k == "solve":
        ret = cz.solve()
        assert ret > 0, "the solve gave up"
    elif k == "sweeps":
        ret = cz.sweeps(st["n"])
        assert ret == st["n"]
    elif k == "set_eps":
        cz.set_eps(st["eps"])
    elif k == "set_itr_max":
        cz.set_itr_max(st["n"])
    elif k == "get_residual":
        dt = W.real(st["dtype"])
        if st["carrier"] is None:
            ret = cz.get_residual(scale=st["scale"])[1]
        else:
            full = np.full(gsz, OUTSIDE, dtype=dt)
            with ctx.on(st["carrier"]):
                if st["carrier"] == "slice":
                    base, out = _based(full, (2, 1, 3), (3, 2, 5))
                elif st["carrier"] in ("c_order", "fortran"):
                    base = out = _carried(ctx, full, st["carrier"])
                else:
                    base = out = ctx.tensor(full, st["carrier"])
                ret = cz.get_residual(out, scale=st["scale"])[1]
                if observe:
                    rec["residual"] = _host(base).tobytes(order="A")
    elif k == "add_field":
        cz.add_field(_part(cz, c, W.correction_data(c, st["seed"], st["dtype"])), st["scale"])
    elif k == "precondition":
        r = W.cycle_data(c, st["seed"])
        if "div" in c:  # (the padded brick, as tests/test_gpu_neumann.py::test_decomposed_solve cuts it)
            loc = cz.local()
            (hi, hj, hk), (ni, nj, nk) = loc["head"], loc["size"]
            r = r[hj - 1:hj - 1 + nj + 2 * PP.G, hi - 1:hi - 1 + ni + 2 * PP.G, hk - 1:hk - 1 + nk + 2 * PP.G]
        z = cz.precondition(r)
        if observe:
            rec["z"] = z.tobytes()
    elif k == "closed_mean":
        ret = cz.closed_mean(st["which"])
    else:
        raise ValueError(k)
    if not observe:
        return None
    rec["ret"] = ret
    if k in ("solve", "sweeps"):
        info = cz.info()
        rec["history"] = list(cz.history())
        rec["info"] = {n: info[n] for n in SOLVE_INFO}
        if k == "solve":
            rec["iter"] = cz.iter
        if field_call_since:
            rec["field_form"] = info["field_form"]
    rec["field"] = _field(cz, c)
    return rec


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for n in a:
        if n == "field":
            assert a[n].tobytes() == b[n].tobytes(), f"{what}: the field differs from the twin's in {int((a[n] != b[n]).sum())} cells"
        else:
            assert a[n] == b[n], f"{what}: {n} differs from the twin's" + ("" if isinstance(a[n], (bytes, list)) else f" ({a[n]} != {b[n]})")


def _twin(ctx, w, i, field):
    """a fresh handle brought to the documented state after step i (-1: a fresh set-up), with the field recorded there"""
    c = w.case
    cz = _new(c)
    if i < 0:
        return cz
    doc = w.docs[i]
    at_step, at, moves = doc["rhs"]
    for name, arg in W.entry(at) if at != "dirichlet" else []:
        getattr(cz, name)(arg)
    _call(ctx, cz, c, dict(w.steps[at_step], carrier="c_order"), at, False, True)
    for m in moves:
        _call(ctx, cz, c, w.steps[m], None, False, True)
    faces, per, closed = W.STATES[doc["state"]]
    info = cz.info()
    assert (info["neumann"], info["periodic"], info["closed"]) == (TN.N.bits(faces), P.bits(per), int(closed)), (w.id, i, info)
    cz.set_eps(doc["eps"])
    cz.set_itr_max(doc["itr_max"])
    cz.set_field(PP.unpad(field))
    return cz


def _segment(ctx, cz, w, i, j):
    """steps i + 1 .. j on a handle, the last one observed"""
    rec = None
    for n in range(i + 1, j + 1):
        since = any(w.steps[m]["kind"] in FIELD_CALLS for m in range(i + 1, n + 1))
        rec = _call(ctx, cz, w.case, w.steps[n], w.docs[n]["state"], n == j, since)
    return rec


def _walk(ctx, w, interleaved):
    """({observed step: record} of the walked handle, [(record, the twin's, what)], this rank's slice of the whole domain); interleaved: the
    twins alive beside it, call by call"""
    c, recs, pairs, last = w.case, {}, [], -1
    cz = _new(c)
    twin = _new(c) if interleaved else None
    sl = cz.global_slice() if "div" in c else None
    try:
        for n, st in enumerate(w.steps):
            since = any(w.steps[m]["kind"] in FIELD_CALLS for m in range(last + 1, n + 1))
            rec = _call(ctx, cz, c, st, w.docs[n]["state"], st["obs"], since)
            if twin is not None:
                rt = _call(ctx, twin, c, st, w.docs[n]["state"], st["obs"], since)
            if st["obs"]:
                recs[n] = rec
                if twin is not None:
                    pairs.append((rec, rt, f"{w.id} step {n} ({st['kind']}), twin alive since step {last}"))
                    twin.close()
                    twin = _twin(ctx, w, n, rec["field"]) if n + 1 < len(w.steps) else None
                last = n
    finally:
        cz.close()
        if twin is not None:
            twin.close()
    return recs, pairs, sl


def _run(w, interleaved):
    """the walk and its twins on the calling thread (a rank of a decomposed walk): what _walk returns, the twins made afterwards included"""
    ctx = _Ctx()
    recs, pairs, sl = _walk(ctx, w, interleaved)
    if not interleaved:
        obs = sorted(recs)
        for i, j in zip([-1] + obs[:-1], obs):
            twin = _twin(ctx, w, i, recs[i]["field"] if i >= 0 else None)
            try:
                rt = _segment(ctx, twin, w, i, j)
            finally:
                twin.close()
            pairs.append((recs[j], rt, f"{w.id} step {j} ({w.steps[j]['kind']}), twin from step {i}"))
    ctx.torch.cuda.synchronize()
    return recs, pairs, sl


def _gathered(w, out, n):
    """the brick [i, j, k] of the whole domain recorded at step n"""
    if "div" not in w.case:
        return PP.unpad(out[0][0][n]["field"])
    X = np.full(w.case["gsz"], np.nan, dtype=W.real(w.case["prec"]))
    for recs, _, sl in out:
        X[sl] = PP.unpad(recs[n]["field"])
    return X


def _anchor(w, out):
    """the last solve against the restatement: the seeded right-hand side of the step before it, the state, the field recorded there"""
    c, n = w.case, len(w.steps) - 1
    doc, g = w.docs[n], out[0][0][n]
    assert w.steps[n]["kind"] == "solve" and w.steps[n - 1]["kind"] == "set_rhs" and doc["rhs"] == (n - 1, doc["state"], ())
    b, p, X = W.rhs_data(c, w.steps[n - 1]["seed"]), _gathered(w, out, n - 1), _gathered(w, out, n)
    # (decomposed: the gathered brick inside zeros, as the family's decomposed tests compare it)
    got = dict(itr=g["ret"], hist=g["history"], P=PP.pad(X) if "div" in c else g["field"], X=X)
    assert g["iter"] == g["ret"]
    if c["solver"] != "pcg":
        TP._compare(c, got, b=b, p=p, eps=doc["eps"], itr_max=doc["itr_max"])
        return
    state = W.STATES[doc["state"]]
    if c["prec"] == "f32":
        o, E, Eh = P.premise_f32(c["gsz"], c["pc"], c["coef"], state, doc["itr_max"], b, p, eps=doc["eps"]), None, None
    else:
        o, E, Eh = P.envelope_f64(c["gsz"], c["pc"], c["coef"], state, doc["itr_max"], b, p, eps=doc["eps"])
    TN._close(c, got, o, E, Eh)


def _mean_anchor(w, n, got):
    """an observed closed_mean(0) against the restated mean of the seeded right-hand side, under the bar of tests/test_gpu_project.py
    (closed_parity.mean_tol; a twin would share a wrong mean)"""
    c, R = w.case, W.real(w.case["prec"])
    at_step, at, _ = w.docs[n]["rhs"]
    st = w.steps[at_step]
    assert W.projections(w, n) == 1
    if st["kind"] == "set_rhs":
        b = W.rhs_data(c, st["seed"])
    else:
        b = J.div(W.velocity_data(c, st["seed"], at), W.STATES[at][1], st["scale"], R)[0]
    inner = b[1:-1, 1:-1, 1:-1]
    m, _, B = CB.mean_of(inner, inner.size, R)
    assert abs(got - float(m)) <= CB.mean_tol(m, B, inner.size), (w.id, n, got, float(m))


TALLIES = {}  # {(walk id, interleaved): the counters of its observed solves, summed}, of the walks that have passed


def _result(wid, interleaved=False):
    """the walk, its twins and the anchors; notes the counters of the walk's observed solves in TALLIES"""
    w = BY_ID[wid]
    c = w.case
    t0 = time.time()
    # torch's HIP runtime up before the library is loaded (test_gpu_neumann._ranks loads it), the order of every single-domain walk and of
    # bench.py: the library then shares that runtime; loaded first and initialised after torch's it finds no device
    TP._torch().cuda.init()
    if "div" in c:
        out =TN._ranks(c["prec"], c["div"], lambda q: _run(w, interleaved))
    else:
        out = [_run(w, interleaved)]
    for q, (_, pairs, _) in enumerate(out):
        for a, b, what in pairs:
            _same(a, b, f"rank {q}: {what}")
    recs = out[0][0]
    for n, r in recs.items():  # what every rank must report alike
        for other, _, _ in out[1:]:
            assert all(other[n].get(k) == r.get(k) for k in ("ret", "history", "iter")), (w.id, n)
        if w.steps[n]["kind"] == "closed_mean" and w.steps[n]["which"] == 0:
            _mean_anchor(w, n, r["ret"])
    t1 = time.time()
    if w.flavour != "named":
        _anchor(w, out)
    tally = {"solves": 0}
    for n, r in recs.items():
        if w.steps[n]["kind"] == "solve":
            tally["solves"] += 1
            for k, v in r["info"].items():
                tally[k] = tally.get(k, 0) + v
    print(f"{w.id}{' interleaved' if interleaved else ''}: {len(recs)} observed steps, walk and twins {t1 - t0:.2f} s, restatement {time.time() - t1:.2f} s, {tally}")
    TALLIES[wid, interleaved] = tally


ALL = W.WALKS["A"] + W.WALKS["B"] + W.WALKS["C"]
BY_ID = {w.id: w for w in ALL + W.NAMED}


@pytest.mark.parametrize("wid", [w.id for w in ALL])
def test_walk_equals_its_twins(wid):
    _result(wid)


@pytest.mark.parametrize("wid", [W.INTERLEAVED[g] for g in "ABC"])
def test_walk_equals_its_twins_alive_beside_it(wid):
    _result(wid, True)


@pytest.mark.parametrize("wid", [w.id for w in W.NAMED])
def test_named_walk_equals_its_twins(wid):
    """the shortest sub-walks that once differed from their twins (tests/walk_plan.py NAMED says what each one found)"""
    _result(wid)


def _sum(walks, key):
    """over the walks of a group, from what test_walk_equals_its_twins noted: a walk that failed there is not run again"""
    missing = [w.id for w in walks if (w.id, False) not in TALLIES]
    assert not missing, f"walks that have not passed test_walk_equals_its_twins in this run: {missing}"
    return sum(TALLIES[w.id, False].get(key, 0) for w in walks)


def test_group_a_ran_the_fused_direction_and_the_cycles():
    for pc, _ in W.A_RUNS:
        ws = [w for w in W.WALKS["A"] if w.case["pc"] == pc]
        assert _sum(ws, "cg_fused") > 0, pc
        if pc != "jacobi":
            assert _sum(ws, "mg_cycles") > 0, pc


def test_group_b_ran_the_fused_passes_and_their_re_runs():
    by = lambda s, pc=None: [w for w in W.WALKS["B"] if w.case["solver"] == s and (pc is None or w.case["pc"] == pc)]  # noqa: E731
    assert _sum(by("jacobi"), "jac3_passes") > 0 or _sum(by("jacobi"), "pass_kind") > 0
    assert _sum(by("sor2sma"), "rb4_passes") > 0
    assert _sum(by("jacobi"), "exact_reruns") >= 2 and _sum(by("sor2sma"), "exact_reruns") >= 2
    assert _sum(by("pbicgstab"), "bicg_fused") > 0


def test_group_c_ran_the_lagged_reduce_and_the_exchanges():
    """every observed solve of the decomposed Jacobi walks in the lagged mode (the third rotation buffer, last_lag, ev_chk[]); the
    decomposed V-cycle exchanged"""
    jac = [w for w in W.WALKS["C"] if w.case["solver"] == "jacobi"]
    assert _sum(jac, "solves") > 0 and _sum(jac, "lagged_reduce") == _sum(jac, "solves")
    assert _sum([w for w in W.WALKS["C"] if w.case["pc"] == "mg"], "mg_exchanges") > 0
