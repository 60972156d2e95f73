"""The committed walks of tests/walk_plan.py, checked without a GPU: the conditions that keep tests/test_gpu_walk.py from being vacuous.
Every condition is derived here from the steps alone (not from the generator's own bookkeeping), and the documented state the generator
carries is checked against a replay of the steps."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import periodic_parity as P  # noqa: E402
import problem_parity as PP  # noqa: E402
import project_parity as J  # noqa: E402
import walk_plan as W  # noqa: E402

ALL = W.WALKS["A"] + W.WALKS["B"] + W.WALKS["C"]
IDS = [w.id for w in ALL]
FRESH = ((0,) * 6, (0,) * 3, False)


def _replay(w):
    """(the state triple after every step, the state name after every step), every setter call checked as it is made"""
    tri, name, out = FRESH, "dirichlet", []
    for st in w.steps:
        if st["kind"] == "state":
            for call, arg in st["calls"]:
                faces, per, closed = tri
                if call == "set_closed_box":
                    tri = ((1,) * 6 if arg else (0,) * 6, per, bool(arg))
                elif call == "set_neumann":
                    assert len(arg) == 6 and not all(arg), (w.id, st)  # (six flags are cz_set_neumann's own refusal)
                    tri = (tuple(arg), per, False)
                else:
                    assert call == "set_periodic" and len(arg) == 3
                    tri = (faces, tuple(arg), closed)
                    assert all(not arg[d] or w.case["gsz"][d] >= 4 for d in range(3)), (w.id, st)
                    assert all(not arg[d] or w.case.get("div", (1, 1, 1))[d] == 1 for d in range(3)), (w.id, st)  # (a cut direction is refused)
                assert P.solvable(*tri), (w.id, st, tri)
            assert tri == W.STATES[st["to"]], (w.id, st, tri)
            name = st["to"]
        out.append((tri, name))
    return out


@pytest.mark.parametrize("w", ALL, ids=IDS)
def test_every_call_is_legal_where_it_is_made(w):
    """24 steps of the group's vocabulary; every setter accepted by periodic_parity.solvable at its moment; periodic directions of four cells
    at least; no projection op under a cut, no boundary state, preconditioner or mean outside pcg; BiCGSTAB never asked for ItrMax 1;
    closed_mean only where the twin can know it"""
    kinds = W.kinds_of(w.case)
    assert len(w.steps) == W.LENGTH == 24 and all(st["kind"] in kinds for st in w.steps)
    states = _replay(w)
    projected = False
    closed_solve = False
    for i, st in enumerate(w.steps):
        tri, name = states[i]
        before = states[i - 1][0] if i else FRESH
        k = st["kind"]
        if w.case["solver"] != "pcg":
            assert tri == FRESH
        if w.case["group"] == "C":
            assert k not in ("set_rhs_div", "sub_grad"), (w.id, i)  # (single domain only)
        if k == "state":
            assert st["to"] != (states[i - 1][1] if i else "dirichlet")
            if tri[2] and not before[2] and projected:  # the closed box a second time over a projected right-hand side: a new one at once
                assert w.steps[i + 1]["kind"] in ("set_rhs", "set_rhs_div"), (w.id, i)
            projected = projected or tri[2]
        elif k in ("set_rhs", "set_rhs_div"):
            projected = tri[2]
            assert 0 <= st["seed"] < 8
        elif k == "set_itr_max":
            assert (2 if w.case["solver"] == "pbicgstab" else 1) <= st["n"] <= 60
        elif k == "set_eps":
            assert st["eps"] in W.EPS["A" if w.case["solver"] == "pcg" else "B"]
        elif k == "sweeps":
            assert 1 <= st["n"] <= 7
        elif k == "closed_mean":
            assert st["which"] in ([0] if projected else []) + ([1, 2] if closed_solve else []), (w.id, i)
        elif k in ("get_residual", "add_field"):
            assert st["scale"] > 0 and st["dtype"] in ("f32", "f64")
        if st["obs"]:
            closed_solve = False
        elif k == "solve" and tri[2]:
            closed_solve = True
    assert [st["kind"] for st in w.steps[:2]] == ["set_rhs", "set_field"]
    tail = w.steps[-W.tail_length(w.case):]
    if len(tail) == 4:  # FP64 pcg: the last solve starts from a seeded field outside the closed mode
        assert [st["kind"] for st in tail] == ["state", "set_field", "set_rhs", "solve"] and not W.STATES[tail[0]["to"]][2]
    else:
        assert [st["kind"] for st in tail] == ["set_itr_max", "set_rhs", "solve"] and (tail[0]["n"] <= W.TAIL_ITR or not PP.krylov(w.case))
    assert all(st["obs"] for st in tail[-2:])


@pytest.mark.parametrize("w", ALL, ids=IDS)
def test_the_documented_state_follows_the_steps(w):
    states = _replay(w)
    eps, itr, rhs = 1e-5, W.ITR_SETUP, None
    for i, (st, doc) in enumerate(zip(w.steps, w.docs)):
        k = st["kind"]
        if k == "set_eps":
            eps = st["eps"]
        elif k == "set_itr_max":
            itr = st["n"]
        elif k in ("set_rhs", "set_rhs_div"):
            rhs = (i, states[i][1], ())
        elif k == "state" and rhs:
            rhs = (rhs[0], rhs[1], rhs[2] + (i,))
        assert doc == dict(state=states[i][1], eps=eps, itr_max=itr, rhs=rhs), (w.id, i)


@pytest.mark.parametrize("w", W.NAMED, ids=[w.id for w in W.NAMED])
def test_named_walks_are_legal_and_documented(w):
    _replay(w)
    test_the_documented_state_follows_the_steps(w)
    assert w.steps[-1]["obs"] and [st["kind"] for st in w.steps[:2]] == ["set_rhs", "set_field"]


def _pairs(walks):
    return {(a["kind"], b["kind"]) for w in walks for a, b in zip(w.steps[:-1], w.steps[1:])}


def test_pair_coverage_group_a():
    """every ordered pair of the twelve op kinds, over the seeds of group A"""
    missing = set(W.all_pairs(W.KINDS_A)) - _pairs(W.WALKS["A"])
    assert len(W.KINDS_A) == 12 and not missing, sorted(missing)


def test_pair_coverage_group_b():
    """every ordered pair of the ten kinds legal on a Dirichlet handle of a stationary or BiCGSTAB solver, over the seeds of group B"""
    missing = set(W.all_pairs(W.KINDS_B)) - _pairs(W.WALKS["B"])
    assert len(W.KINDS_B) == 10 and not missing, sorted(missing)


def _transitions(w):
    """the ordered pairs (s, t) of a walk with a solve in s during the stay before the transition and a solve in t after it with no
    right-hand side or field brought in between"""
    got, solved, pending = set(), False, None
    name = "dirichlet"
    for st in w.steps:
        k = st["kind"]
        if k == "state":
            pending = (name, st["to"]) if solved else None
            name, solved = st["to"], False
        elif k in W.IMPORTS:
            pending = None
        elif k == "solve":
            solved = True
            if pending:
                got.add(pending)
                pending = None
    return got


@pytest.mark.parametrize("pc", [pc for pc, _ in W.A_RUNS])
def test_transition_coverage(pc):
    """all 42 ordered pairs of distinct boundary states, each with a solve before it and a solve on what it left behind, per preconditioner"""
    got = set()
    for w in W.WALKS["A"]:
        if w.case["pc"] == pc:
            got |= _transitions(w)
    want = {(s, t) for s in W.NAMES for t in W.NAMES if s != t}
    assert len(want) == 42 and not want - got, sorted(want - got)


@pytest.mark.parametrize("pc", [pc for pc, _ in W.A_RUNS])
def test_the_mean_of_the_rhs_is_observed(pc):
    """a twin runs the same library, so a closed_mean that both sides get wrong alike stays equal: the GPU test also compares every observed
    closed_mean(0) with the restated mean of the seeded right-hand side.  Per preconditioner at least two such steps, and the right-hand
    side behind each was projected exactly once (its mean is the mean of the seeded array)"""
    seen = 0
    for w in W.WALKS["A"]:
        if w.case["pc"] != pc:
            continue
        for n, st in enumerate(w.steps):
            if st["kind"] == "closed_mean" and st["which"] == 0:
                assert W.projections(w, n) == 1, (w.id, n)
                seen += st["obs"]
    assert seen >= 2, seen


@pytest.mark.parametrize("w", ALL, ids=IDS)
def test_an_unobserved_run_holds_a_side_stream_import_followed_by_solve(w):
    ok = False
    for i in range(len(w.steps) - 1):
        a, b = w.steps[i], w.steps[i + 1]
        if not a["obs"] and not b["obs"] and a["kind"] in ("set_rhs", "set_field", "set_rhs_div") and a.get("carrier") == "device_side" and b["kind"] == "solve":
            ok = True
    assert ok, w.id
    assert 6 <= sum(st["obs"] for st in w.steps) <= 20, w.id  # about half of the steps


C_PCG = sorted({w.case["id"] for w in W.WALKS["C"] if w.case["solver"] == "pcg"})


@pytest.mark.parametrize("cid", C_PCG)
def test_transition_coverage_decomposed(cid):
    """group C, per pcg case: every ordered pair of distinct states among those whose periodic directions its division leaves whole --
    (2, 1, 1): dirichlet, inflow, closed; (1, 2, 2): also px -- with a solve before it and a solve on what it left behind"""
    ws = [w for w in W.WALKS["C"] if w.case["id"] == cid]
    div = ws[0].case["div"]
    names = [n for n in W.NAMES if not any(W.STATES[n][1][d] and div[d] > 1 for d in range(3))]
    assert names == {(2, 1, 1): ["dirichlet", "inflow", "closed"], (1, 2, 2): ["dirichlet", "inflow", "closed", "px"]}[div]
    got = set().union(*[_transitions(w) for w in ws])
    want = {(s, t) for s in names for t in names if s != t}
    assert not want - got, sorted(want - got)


def test_the_groups_cover_their_table():
    """group A: three preconditioners x two precisions x two boxes; group B: every Dirichlet family named; group C: pcg mg and Jacobi
    (FP32, FP64) on both divisions; the interleaved walks exist"""
    c = {(w.case["solver"], w.case["pc"], w.case["prec"], w.case["div"]) for w in W.WALKS["C"]}
    assert c == {(s, pc, q, d) for s, pc, q in (("pcg", "mg", "f64"), ("jacobi", None, "f32"), ("jacobi", None, "f64")) for d in ((2, 1, 1), (1, 2, 2))}
    assert all(w.case["itr_max"] == 60 and w.case["gsz"][d] % w.case["div"][d] == 0 for w in W.WALKS["C"] for d in range(3))
    a = {(w.case["pc"], w.case["prec"], w.case["gsz"]) for w in W.WALKS["A"]}
    assert a == {(pc, q, g) for pc, _ in W.A_RUNS for q in ("f32", "f64") for g in W.A_BOXES}
    b = {(w.case["solver"], w.case["pc"]) for w in W.WALKS["B"]}
    assert b == {("jacobi", None), ("sor2sma", None), ("psor", None), ("pcr_rb", None), ("pcr", None), ("pbicgstab", "jacobi"), ("pbicgstab", "sor2sma")}
    assert len({w.id for w in ALL}) == len(ALL)
    for g in "ABC":
        assert W.INTERLEAVED[g] in [w.id for w in W.WALKS[g]]
    w0 = W.Walk(ALL[-1].case, ALL[-1].seed, ALL[-1].share, ALL[-1].flavour, ALL[-1].primary)
    assert w0.steps == ALL[-1].steps and w0.docs == ALL[-1].docs  # deterministic


# ---- the stationary walks of group B through the oracle: the solves land where the fused passes' bookkeeping is at stake
def oracle_solves(w):
    """[(iterations, converged, itr_max)] of the walk's solves, by problem_parity.run chained as problem_parity.resolve chains two solves"""
    c = w.case
    R = W.real(c["prec"])
    b = p = None
    eps, itr_max, out = 1e-5, W.ITR_SETUP, []
    for st in w.steps:
        k = st["kind"]
        if k == "set_rhs":
            b = W.rhs_data(c, st["seed"])
        elif k == "set_field":
            p = W.field_data(c, st["seed"])
        elif k == "set_rhs_div":
            b = J.div(W.velocity_data(c, st["seed"], "dirichlet"), P.NOPER, st["scale"], R)[0]
        elif k == "add_field":
            e = W.correction_data(c, st["seed"], st["dtype"]).astype(R)
            p = p.copy()
            p[1:-1, 1:-1, 1:-1] = p[1:-1, 1:-1, 1:-1] + e[1:-1, 1:-1, 1:-1] * R(st["scale"])
        elif k == "set_eps":
            eps = st["eps"]
        elif k == "set_itr_max":
            itr_max = st["n"]
        elif k == "sweeps":
            p = PP.unpad(PP.run(c, b=b, p=p, eps=-1.0, itr_max=st["n"]).P)
        elif k == "solve":
            o = PP.run(c, b=b, p=p, eps=eps, itr_max=itr_max)
            p = PP.unpad(o.P)
            out.append((o.itr, bool(o.res < eps), itr_max))
    return out


STATIONARY = [w for w in W.WALKS["B"] if w.case["solver"] in ("jacobi", "sor2sma")]


@pytest.mark.parametrize("w", STATIONARY, ids=[w.id for w in STATIONARY])
def test_mid_pass_convergence(w):
    """at least three solves converge below itr_max, two of them at a count that is odd and no multiple of 3 (not the last iteration of a
    fused pass of two or of three: the re-run path), and one ends at itr_max unconverged"""
    s = oracle_solves(w)
    early = [itr for itr, conv, n in s if conv and itr < n]
    print(w.id, s)
    assert len(early) >= 3, s
    assert sum(1 for itr in early if itr % 2 == 1 and itr % 3 != 0) >= 2, s
    assert any(itr >= n and not conv for itr, conv, n in s), s  # (the oracle's loop leaves its counter at itr_max + 1 there)
