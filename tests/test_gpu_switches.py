"""GPU tests (-m gpu) of every configuration switch on the route a user takes: the variable in the environment of a fresh process
(tests/switch_worker.py), parsed by czhip_init, CZ::CZ or cz_comm.cpp, then whole solves.  tests/switch_table.py holds the table (SWITCHES) and
says what every leg is held to; this file runs the children -- one at a time, each under its own time limit; after an abort, a signal or a
time-out every later test of the file fails without starting another child -- and checks

* that the other path ran: launch counts per timing label, cz_info, and what the parse made of the value (czhip_tuning_describe,
  cz_config_in_force);
* stationary solvers against the wide-accumulating oracle: field bit for bit, iteration count equal, history and res to the bars of
  test_gpu_convergence_landing.py;
* Krylov solvers byte for byte against the default-environment leg, which test_default_leg holds to the exact-dot oracle bit for bit.

Two setters no other test calls, czhip_set_psor_ahead and czhip_set_comm_cus, are checked in this process against the oracle."""
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

from oracle import cz_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import switch_table as T  # noqa: E402
from switch_worker import case_args  # noqa: E402
from test_gpu_convergence_landing import _check_run  # noqa: E402

pytestmark = pytest.mark.gpu
WORKER = os.path.join(HERE, "switch_worker.py")
_dead = []          # why no further child may start
_cache = {}         # ("default" | "oracle", case) -> record


def _child(env, cases, abi=False):
    """one child process with `env` on top of this process's environment (every switch of the table removed first); returns its records with
    the fields loaded"""
    if _dead:
        pytest.fail(f"no further child is started: {_dead[0]}")
    e = {k: v for k, v in os.environ.items() if k not in {r["var"] for r in T.SWITCHES}}
    e.update(env)
    limit = T.child_timeout(cases, abi)
    with tempfile.TemporaryDirectory(prefix="cz_switch_") as out:
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, WORKER, out, json.dumps(dict(cases=list(cases), abi=abi))], env=e, capture_output=True, text=True,
                               timeout=limit)
        except subprocess.TimeoutExpired:
            _dead.append(f"the child of {env} ran into its time limit of {limit:.0f} s")
            pytest.fail(_dead[0])
        wall = time.time() - t0
        if r.returncode < 0 or r.returncode in (134, 139):
            _dead.append(f"the child of {env} ended with status {r.returncode}: {r.stderr[-1500:]}")
            pytest.fail(_dead[0])
        assert r.returncode == 0, f"child of {env} failed (exit {r.returncode}):\n{r.stdout[-1500:]}\n{r.stderr[-4000:]}"
        with open(os.path.join(out, "result.json")) as f:
            res = json.load(f)
        for name, rec in res["cases"].items():
            rec["P"] = np.load(os.path.join(out, name + ".npy"))
    res["wall_s"] = wall
    print(f"child {env or 'default'}: {wall:.1f} s, cases " + ", ".join(f"{n} {rec['wall_s']:.2f}" for n, rec in res["cases"].items())
          + (f", abi {res['abi']['wall_s']:.1f} ({res['abi']['ran']} checks)" if "abi" in res else ""))
    return res


def _default(cases):
    """the default-environment records of `cases` (one child for all that are still missing)"""
    missing = [n for n in cases if ("default", n) not in _cache]
    if missing:
        res = _child({}, missing)
        assert res["config_set"].strip() == "" or not any(r["var"] in res["config_set"] for r in T.SWITCHES), res["config_set"]
        for n in missing:
            _cache["default", n] = res["cases"][n]
    return {n: _cache["default", n] for n in cases}


def _oracle(name):
    if ("oracle", name) not in _cache:
        c = T.CASES[name]
        prec, gsz, solver, itr_max, coef, pc, div = case_args(c)
        if c["family"] == "stationary":
            o = O.run(gsz, solver, itr_max, coef, None, kind="oracle", prec=prec, wide=True)
        else:
            m = importlib.import_module(c["module"])
            o = m.oracle(next(x for x in m.CASES if x["id"] == c["id"]), itr_max)
        _cache["oracle", name] = o
    return _cache["oracle", name]


def _check_stationary(name, rec, counters):
    """the bars of test_gpu_convergence_landing.py on one record (decomposed: every rank's, and the assembled inner field)"""
    c, o = T.CASES[name], _oracle(name)
    if c["iter"] is not None:
        assert o.itr == c["iter"], (name, o.itr)  # the fixture still describes the oracle
    lc = dict(name=name, iter=o.itr, solver=c["solver"], gsz=list(c["gsz"]), counters=c["counters"] if counters else {})
    print(f"{name}: itr {rec['itr']} (oracle {o.itr}), res {rec['res']:.17g} (oracle {o.res:.17g}), rel {abs(rec['res'] - o.res) / o.res:.3g}")
    if c["div"]:
        for r in rec["ranks"]:
            _check_run(lc, o, r["itr"], r["res"], r["history"], None, r["info"])
        inner = (slice(2, -2),) * 3
        assert rec["P"][inner].tobytes() == o.P[inner].tobytes(), f"{name}: field differs from the oracle"
    else:
        _check_run(lc, o, rec["itr"], rec["res"], rec["history"], rec["P"], rec["info"])
        if "get_field_equals_field" in rec:
            assert rec["get_field_equals_field"], f"{name}: cz_get_field differs from cz_field"


def _check_krylov_default(name, rec):
    """FP32, premise checked on the CPU: field, history and count equal the exact-dot oracle's bit for bit"""
    c, o = T.CASES[name], _oracle(name)
    assert rec["itr"] == o.itr, (name, rec["itr"], o.itr)
    assert rec["history"] == [r for _, r in o.history], (name, rec["history"], o.history)
    if c["div"]:
        assert all(r["itr"] == rec["itr"] and r["history"] == rec["history"] for r in rec["ranks"]), name
        assert rec["P"][2:-2, 2:-2, 2:-2].tobytes() == o.P[2:-2, 2:-2, 2:-2].tobytes(), f"{name}: field differs from the exact-dot oracle"
    else:
        assert rec["P"].tobytes() == o.P.tobytes(), f"{name}: field differs from the exact-dot oracle"


def _rule(rule, rec, dflt, what, ctx):
    """one expectation of a row: an int, or a named rule"""
    got = what(rec)
    if isinstance(rule, int):
        assert got == rule, (ctx, got, rule)
    elif rule == ">0":
        assert got > 0, (ctx, got)
    elif rule == "sweeps":
        assert len(rec["history"]) <= got <= len(rec["history"]) + 64, (ctx, got, len(rec["history"]))
    elif rule == "default":
        assert got == what(dflt), (ctx, got, what(dflt))
    elif rule == ">default":
        assert got > what(dflt), (ctx, got, what(dflt))
    elif rule == "clamped":  # reserve_comm_cus: at most half the CUs of an XCD, on the 8-XCD part
        per_xcd = rec["tuning"]["num_cu"] // 8
        asked = int(ctx[0].split("=")[1])
        want = 0 if rec["tuning"]["num_cu"] % 8 or per_xcd < 4 else max(0, min(asked, per_xcd // 2))
        assert got == want, (ctx, got, want)
    elif rule == "gather_level":
        from cubez_amd import decomp as D
        c = T.CASES[ctx[1]]
        gsz = case_args(c)[1]
        want = D.mg_gather_level(gsz, c["div"], gather_points=int(ctx[0].split("=")[1]))
        assert got == want and got != what(dflt), (ctx, got, want, what(dflt))
    else:
        raise AssertionError(f"unknown rule {rule!r}")


def _ranks(rec):
    return rec.get("ranks") or [rec]


def _check_leg(row, res, dflt):
    for name in row["cases"]:
        rec, d = res["cases"][name], dflt[name]
        # -- the switch arrived and was parsed as the table says
        for r in _ranks(rec):
            for k, v in row.get("tuning", {}).items():
                _rule(v, r, _ranks(d)[0], lambda x, k=k: x["tuning"][k], (row["id"], name, "tuning", k))
            for k, v in row.get("in_force", {}).items():
                _rule(v, r, _ranks(d)[0], lambda x, k=k: x["in_force"][k], (row["id"], name, "in_force", k))
        # -- the other path ran
        for r, dr in zip(_ranks(rec), _ranks(d)):
            for k, v in {**row.get("launch", {}).get("*", {}), **row.get("launch", {}).get(name, {})}.items():
                _rule(v, r, dr, lambda x, k=k: x["launches"][k], (row["id"], name, "launches", k))
            for k, v in {**row.get("info", {}).get("*", {}), **row.get("info", {}).get(name, {})}.items():
                _rule(v, r, dr, lambda x, k=k: x["info"][k], (row["id"], name, "info", k))
        # -- and computed what it must
        if T.CASES[name]["family"] == "stationary":
            _check_stationary(name, rec, counters=name in row.get("counters", []))
        else:
            assert rec["itr"] == d["itr"], (row["id"], name, rec["itr"], d["itr"])
            assert rec["history"] == d["history"], (row["id"], name, "history differs from the default leg", rec["history"], d["history"])
            assert rec["P"].tobytes() == d["P"].tobytes(), (row["id"], name, "field differs from the default leg")
    if row.get("abi"):
        assert res["abi"]["ran"] > 0


def test_default_leg():
    """the default environment: every case takes the path its fixture names and equals its oracle; no switch of the table is set"""
    dflt = _default(T.DEFAULT_CASES)
    for name, rec in dflt.items():
        print(name, "launches", {k: v for k, v in rec["launches"].items() if v}, "info", {k: v for k, v in rec["info"].items() if v})
        if T.CASES[name]["family"] == "stationary":
            _check_stationary(name, rec, counters=True)
        else:
            _check_krylov_default(name, rec)
    t = dflt["jacobi_pair_sweep1_poll_last"]["tuning"]
    assert (t["fuse_fin"], t["use_t2"], t["rb4"], t["jac3"], t["unit_coef"], t["t2_map"], t["psor_ahead"], t["cu_reserved"]) == (1, 1, 1, 1, 1, 1, 0, 0), t
    d = dflt["jacobi_decomposed_1x2x2_lag1_sweep1"]
    assert all(r["in_force"]["comm_pack_j"] == 0 and r["in_force"]["comm_direct_messages"] > 0 and r["in_force"]["comm_cus"] == 2 for r in d["ranks"]), d["ranks"]
    assert dflt["pcg_mg"]["launches"]["mg_tail"] > 0 and dflt["pcg_jacobi"]["info"]["cg_fused"] > 0


def test_default_abi_checks():
    """the C-ABI checks the CZHIP_FUSE_FIN=0 and CZHIP_T2=0 legs repeat, in the default environment (their time is the base of those legs' limit)"""
    res = _child({}, [], abi=True)
    assert res["abi"]["ran"] > 0


LEGS = [r for r in T.SWITCHES if not r.get("rccl")]


@pytest.mark.parametrize("row", LEGS, ids=[r["id"] for r in LEGS])
def test_switch_leg(row):
    dflt = _default([n for n in row["cases"] if n in T.DEFAULT_CASES])
    res = _child(row["env"], row["cases"], abi=bool(row.get("abi")))
    for k, v in row["env"].items():
        assert f"{k}={v}\n" in res["config_set"], res["config_set"]
    # (cases that exist for one leg only have no default record: rules against the default are not used on them)
    _check_leg(row, res, {n: dflt.get(n, res["cases"][n]) for n in row["cases"]})


# ---- the RCCL-only legs: two ranks (processes) on the one GPU, J faces between them
def _rccl(extra):
    from test_gpu_rccl import run_ranks
    if _dead:
        pytest.fail(f"no further child is started: {_dead[0]}")
    prec, gsz, solver, itmax, coef, div = T.RCCL_CASE
    t0 = time.time()
    recs, G, logs = run_ranks(prec, gsz, solver, itmax, coef, div, extra_env=extra, timeout=max(60.0, 10.0 * T.RCCL_SECONDS))
    print(f"rccl ranks {extra or 'default'}: {time.time() - t0:.1f} s")
    o = O.run(gsz, solver, itmax, coef, None, kind="oracle", prec=prec, wide=True)
    assert G[2:-2, 2:-2, 2:-2].tobytes() == o.P[2:-2, 2:-2, 2:-2].tobytes(), "field differs from the oracle"
    for rec in recs:
        assert rec["itr"] == o.itr and rec["info"]["rccl_ranks"] == 2, rec["info"]
        assert np.allclose(rec["history"], [r for _, r in o.history], rtol=1e-10, atol=0)
        assert abs(rec["res"] - o.res) <= 1e-10 * o.res
    return recs


def test_rccl_default_leg():
    for rec in _rccl({}):
        assert rec["in_force"]["comm_one_comm"] == 0 and rec["in_force"]["comm_pack_j"] == 0 and rec["in_force"]["comm_direct_messages"] > 0, rec["in_force"]


@pytest.mark.parametrize("row", T.RCCL_ROWS, ids=[r["id"] for r in T.RCCL_ROWS])
def test_rccl_switch_leg(row):
    for rec in _rccl(row["env"]):
        for k, v in row["in_force"].items():
            assert rec["in_force"][k] == v, (row["id"], k, rec["in_force"])


# ---- two setters no other test calls
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("nk", [40, 330], ids=["nk_below_300", "nk_above_300"])
def test_psor_ahead_setter_gives_the_oracles_bits(prec, nk):
    """czhip_set_psor_ahead(4 | 8 | 0): face words asked for 4 or 8 steps ahead (the launcher's rule switches at 300 points along k in FP32);
    psor_ and psor_maf_ give the oracle's field bit for bit and its wide sum either way; the setter returns the previous value"""
    from cubez_amd import CzHip
    h, ko = CzHip(prec), O.Kernels("oracle", prec)
    ni, nj = 9, 7
    sz, idx = [ni, nj, nk], [2, ni - 1, 2, nj - 1, 2, nk - 1]
    rng = np.random.default_rng(nk)
    p0, b0 = (rng.uniform(-1, 1, (nj + 4, ni + 4, nk + 4)).astype(ko.real) for _ in range(2))
    cf = [1.1, 0.9, 1.05, 0.95, 1.2, 0.8, 6.3]
    xc, yc, zc = (np.cumsum(rng.uniform(0.5, 1.5, n + 4)).astype(ko.real) for n in (ni, nj, nk))
    p1, w1 = p0.copy(), np.zeros(1)
    ko.psor(p1, sz, idx, cf, 1.2, b0, wide=w1)
    p2, w2 = p0.copy(), np.zeros(1)
    ko.psor_maf(p2, sz, idx, xc, yc, zc, 1.2, b0, wide=w2)
    before = h.lib.czhip_set_psor_ahead(0)
    try:
        prev = 0
        for steps in (4, 8, 0):
            assert h.lib.czhip_set_psor_ahead(steps) == prev
            assert h.tuning()["psor_ahead"] == steps
            prev = steps
            dp, db = h.alloc(sz, p0), h.alloc(sz, b0)
            r = h.psor(dp, sz, idx, cf, 1.2, db)
            assert dp.get().tobytes() == p1.tobytes(), steps
            assert abs(r - w1[0]) <= 1e-12 * w1[0], (steps, r, w1[0])
            dq = h.alloc(sz, p0)
            r = h.psor_maf(dq, sz, idx, xc, yc, zc, 1.2, db)
            assert dq.get().tobytes() == p2.tobytes(), steps
            assert abs(r - w2[0]) <= 1e-12 * w2[0], (steps, r, w2[0])
            for a in (dp, db, dq):
                a.free()
        assert h.lib.czhip_set_psor_ahead(5) == 0 and h.tuning()["psor_ahead"] == 0  # any other value is not taken
    finally:
        h.lib.czhip_set_psor_ahead(before)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_comm_cus_setter_round_trips_and_the_pass_planned_under_it_equals_the_oracle(prec):
    """czhip_set_comm_cus(k) returns the reservation in force (at most half an XCD's CUs) and czhip_tuning_describe shows it; a fused pass planned
    under each reservation -- 40 x 36 x 61 and the k-windowed 9 x 7 x 1100 -- gives two oracle sweeps bit for bit and their wide sums"""
    from cubez_amd import CzHip
    h, ko = CzHip(prec), O.Kernels("oracle", prec)
    per_xcd = h.tuning()["num_cu"] // 8
    try:
        for k in (0, 1, 2, 4, per_xcd // 2, per_xcd):
            want = min(k, per_xcd // 2) if h.tuning()["num_cu"] % 8 == 0 and per_xcd >= 4 else 0
            assert h.lib.czhip_set_comm_cus(k) == want and h.tuning()["cu_reserved"] == want, (k, want, h.tuning())
            for ni, nj, nk in ((40, 36, 61), (9, 7, 1100)):
                sz, idx = [ni, nj, nk], [2, ni - 1, 2, nj - 1, 2, nk - 1]
                rng = np.random.default_rng(ni + nk)
                p, b = (rng.uniform(-1, 1, (nj + 4, ni + 4, nk + 4)).astype(ko.real) for _ in range(2))
                cf = rng.uniform(0.6, 1.0, 7).astype(ko.real)
                cf[6] = 6.2
                a, wk, sums = p.copy(), np.zeros_like(p), []
                for _ in range(2):
                    w = np.zeros(1)
                    ko.jacobi(a, sz, idx, cf, 0.9, b, wk, wide=w)
                    sums.append(w[0])
                du, dw, db = h.alloc(sz, p), h.alloc(sz, p), h.alloc(sz, b)
                ok, r0, r1 = h.jacobi2(du, dw, db, sz, idx, cf, 0.9)
                assert ok, (k, sz)
                assert dw.get().tobytes() == a.tobytes(), (k, sz)
                assert abs(r0 - sums[0]) <= 1e-11 * sums[0] and abs(r1 - sums[1]) <= 1e-11 * sums[1], (k, sz, r0, r1, sums)
                for d in (du, dw, db):
                    d.free()
    finally:
        h.lib.czhip_set_comm_cus(0)
