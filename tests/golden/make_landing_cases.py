#!/usr/bin/env python3
"""Generate landing_cases.json: stationary solves whose converged iteration lands on a chosen position of the device-side pass protocol.

The GPU driver runs Jacobi and red-black SOR as launches of one, two or three iterations (pairs, jac3 triples, rb4 passes); the last
workgroup of each launch tests convergence, later launches skip, the host looks at the flag every POLL_EVERY iterations through a copy two
polls old, and a launch whose converged iteration is not its last is re-run from its input.  Each case here is a (grid, coefficient) that
the oracle (the C restatement, wide residuals, on the CPU) converges at an iteration with the wanted position: the first, second or third
iteration of a launch, the last launch before a host poll or the first after it, an ItrMax equal to the converged iteration or one short of
it, decomposed passes.  The host loop of the driver (cubez_amd/csrc/cz_driver.cpp, CZ::JACOBI / CZ::RBSOR with FlagPoll) is restated below
to predict the info() counters each case must show: exact_reruns, jac3_passes, rb4_passes.

Every residual of every case lies at least MARGIN (relative) away from eps, so no summation order can move the converged iteration
(tests/test_landing_cases.py re-checks that premise on a few cases).  Deterministic: running it twice gives the same file.

    python tests/golden/make_landing_cases.py
"""
import json
import os
import sys

os.environ.setdefault("OMP_NUM_THREADS", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

from oracle import cz_oracle as O  # noqa: E402

OUT = os.path.join(HERE, "landing_cases.json")
POLL_EVERY = 32   # cz_driver: the host polls after every POLL_EVERY / 2 Jacobi launches, after every POLL_EVERY red-black iterations
MARGIN = 1e-9
ITR_BIG = 100000
GRIDS = [(16, 16, 16), (16, 16, 18), (18, 16, 16), (16, 18, 16), (16, 18, 20), (20, 16, 18), (18, 20, 16), (17, 16, 19), (19, 17, 16),
         (16, 20, 20), (20, 20, 16), (18, 18, 18)]


def coefs(lo, hi, step):
    n = int(round((hi - lo) / step))
    return [round(lo + i * step, 3) for i in range(n + 1)]


def jacobi_host(conv, itr_max, mode):
    """CZ::JACOBI's launches (mode single | pair | triple): returns (Iter, exact_reruns, jac3_passes)"""
    itr, launches, flags, stop = 1, [], [], False
    while itr <= itr_max and not stop:
        done = 1
        if mode != "single" and itr + 1 <= itr_max:
            done = 3 if (mode == "triple" and itr_max >= 3 and itr + 2 <= itr_max) else 2
        launches.append((itr, done))
        itr += done
        if len(launches) % (POLL_EVERY // 2) == 0 and itr <= itr_max:  # FlagPoll::stop: the copy of two polls back
            flags.append(conv is not None and conv <= itr - 1)
            stop = len(flags) >= 3 and flags[-3]
    return _end(conv, itr_max, launches) + (sum(1 for _, n in launches if n == 3),)


def rbsor_host(conv, itr_max, rb4):
    """CZ::RBSOR's launches (one iteration each, or rb4 passes of two): returns (Iter, exact_reruns, rb4_passes)"""
    itr, launches, flags, stop = 1, [], [], False
    while itr <= itr_max and not stop:
        done = 2 if (rb4 and itr + 1 <= itr_max) else 1
        launches.append((itr, done))
        last = itr + done - 1
        poll_now = last // POLL_EVERY > (itr - 1) // POLL_EVERY
        itr += done
        if poll_now and last < itr_max:
            flags.append(conv is not None and conv <= last)
            stop = len(flags) >= 3 and flags[-3]
    return _end(conv, itr_max, launches) + (sum(1 for _, n in launches if n == 2),)


def _end(conv, itr_max, launches):
    """fused_end: Iter, and whether the launch holding the converged iteration had to be re-run"""
    if conv is None or conv > itr_max:
        return itr_max + 1, 0
    for first, n in launches:
        if first <= conv < first + n:
            return conv, 1 if conv < first + n - 1 else 0
    raise AssertionError("converged iteration never launched")


def oracle(gsz, solver, itr_max, coef, prec):
    o = O.run(gsz, solver, itr_max, coef, None, kind="oracle", prec=prec, wide=True)
    return o.itr, [r for _, r in o.history]


def margin_ok(hist):
    return all(abs(r - O.EPS) >= MARGIN * O.EPS for r in hist)


def launch_of(conv, per):
    """1-based index of the launch (all of `per` iterations) that holds iteration conv"""
    return (conv + per - 1) // per


# (name, solver, prec, mode, coefficient range, predicate on the converged iteration c)
SEARCH = [
    # Jacobi, one sweep per launch (the two-stage pass off): the host polls after every 16 launches
    ("jacobi_single_poll_last", "jacobi", "f32", "single", (0.6, 1.0, 0.01), lambda c: c % 16 == 0),
    ("jacobi_single_poll_first", "jacobi", "f64", "single", (0.6, 1.0, 0.01), lambda c: c % 16 == 1),
    # pairs (jac3 off): converged on the first sweep (re-run) or the second, in the last launch before a poll, the first after it, or between
    ("jacobi_pair_sweep1_poll_last", "jacobi", "f32", "pair", (0.6, 1.0, 0.01), lambda c: c % 2 == 1 and launch_of(c, 2) % 16 == 0),
    ("jacobi_pair_sweep1_poll_first", "jacobi", "f64", "pair", (0.6, 1.0, 0.01), lambda c: c % 2 == 1 and launch_of(c, 2) % 16 == 1),
    ("jacobi_pair_sweep2_poll_last", "jacobi", "f64", "pair", (0.6, 1.0, 0.01), lambda c: c % 2 == 0 and launch_of(c, 2) % 16 == 0),
    ("jacobi_pair_sweep2_poll_first", "jacobi", "f32", "pair", (0.6, 1.0, 0.01), lambda c: c % 2 == 0 and launch_of(c, 2) % 16 == 1),
    ("jacobi_pair_sweep1_mid", "jacobi", "f32", "pair", (0.6, 1.0, 0.01), lambda c: c % 2 == 1 and launch_of(c, 2) % 16 == 8),
    # triples (jac3 forced on): sweep 1 (one sweep re-run), 2 (one pair re-run), 3 (nothing)
    ("jacobi_triple_sweep1_poll_last", "jacobi", "f32", "triple", (0.6, 1.0, 0.01), lambda c: c % 3 == 1 and launch_of(c, 3) % 16 == 0),
    ("jacobi_triple_sweep1_poll_first", "jacobi", "f64", "triple", (0.6, 1.0, 0.01), lambda c: c % 3 == 1 and launch_of(c, 3) % 16 == 1),
    ("jacobi_triple_sweep2_poll_last", "jacobi", "f64", "triple", (0.6, 1.0, 0.01), lambda c: c % 3 == 2 and launch_of(c, 3) % 16 == 0),
    ("jacobi_triple_sweep2_poll_first", "jacobi", "f32", "triple", (0.6, 1.0, 0.01), lambda c: c % 3 == 2 and launch_of(c, 3) % 16 == 1),
    ("jacobi_triple_sweep3_poll_last", "jacobi", "f32", "triple", (0.6, 1.0, 0.01), lambda c: c % 3 == 0 and launch_of(c, 3) % 16 == 0),
    ("jacobi_triple_sweep3_mid", "jacobi", "f64", "triple", (0.6, 1.0, 0.01), lambda c: c % 3 == 0 and launch_of(c, 3) % 16 == 8),
    # red-black SOR, one iteration per pass (rb4 off): the host polls after every 32 iterations
    ("sor2sma_one_poll_last", "sor2sma", "f32", "rb1", (1.2, 1.9, 0.01), lambda c: c % 32 == 0),
    ("sor2sma_one_poll_first", "sor2sma", "f64", "rb1", (1.2, 1.9, 0.01), lambda c: c % 32 == 1),
    # rb4 (forced on): iteration 1 of a pass (re-run) or 2, the pass ending at a poll or starting after one
    ("sor2sma_rb4_iter1_poll_last", "sor2sma", "f32", "rb4", (1.2, 1.9, 0.01), lambda c: c % 2 == 1 and c % 32 == 31),
    ("sor2sma_rb4_iter1_poll_first", "sor2sma", "f64", "rb4", (1.2, 1.9, 0.01), lambda c: c % 2 == 1 and c % 32 == 1),
    ("sor2sma_rb4_iter2_poll_last", "sor2sma", "f64", "rb4", (1.2, 1.9, 0.01), lambda c: c % 2 == 0 and c % 32 == 0),
    ("sor2sma_rb4_iter2_mid", "sor2sma", "f32", "rb4", (1.2, 1.9, 0.01), lambda c: c % 2 == 0 and c % 32 == 16),
    # the MAF pair (two jacobi_maf sweeps / one red-black iteration per launch)
    ("jacobi_maf_sweep1", "jacobi_maf", "f64", "pair", (0.6, 1.0, 0.01), lambda c: c % 2 == 1),
    ("jacobi_maf_sweep2", "jacobi_maf", "f32", "pair", (0.6, 1.0, 0.01), lambda c: c % 2 == 0),
    ("sor2sma_maf", "sor2sma_maf", "f64", "rb1", (1.2, 1.9, 0.01), lambda c: True),
    # lexicographic point SOR and the red-black line SOR: one iteration per launch, host polls every 32 / every iteration
    ("psor_poll_last", "psor", "f64", "plain", (1.2, 1.9, 0.01), lambda c: c % 32 == 0),
    ("pcr_rb", "pcr_rb", "f32", "plain", (1.1, 1.5, 0.01), lambda c: True),
]

# ItrMax at or just below the converged iteration of a found case: (name, base case, ItrMax - Iter, predicate on Iter)
ITRMAX = [
    ("jacobi_triple_itrmax_equal", "triple", "f64", 0, lambda c: c % 3 == 1),      # last launch: one sweep after the triples
    ("jacobi_triple_itrmax_short", "triple", "f32", -1, lambda c: c % 3 == 0),     # ItrMax ends the middle of a triple: a pair last
    ("jacobi_triple_itrmax_short_single", "triple", "f64", -1, lambda c: c % 3 == 2),  # ... one sweep last
    ("jacobi_pair_itrmax_equal", "pair", "f32", 0, lambda c: c % 2 == 1),
    ("jacobi_pair_itrmax_short", "pair", "f64", -1, lambda c: c % 2 == 0),
    ("sor2sma_rb4_itrmax_equal", "rb4", "f32", 0, lambda c: c % 2 == 1),            # ItrMax ends the middle of an rb4 pass
    ("sor2sma_rb4_itrmax_short", "rb4", "f64", -1, lambda c: c % 2 == 0),
]

# decomposed Jacobi through the LOCAL transport, converging on the first sweep of a SPLIT pair (re-run; lagged: three rotating buffers)
DECOMP = [((2, 1, 1), 0), ((2, 1, 1), 1), ((1, 2, 2), 0), ((1, 2, 2), 1)]


def counters(solver, mode, conv, itr_max):
    if solver.startswith("jacobi"):
        it, rer, deep = jacobi_host(conv, itr_max, mode if mode in ("single", "pair", "triple") else "pair")
        return it, dict(exact_reruns=rer, jac3_passes=deep, rb4_passes=0, pass_kind=0 if mode == "single" else 1)
    if solver.startswith("sor2sma"):
        it, rer, deep = rbsor_host(conv, itr_max, mode == "rb4")
        return it, dict(exact_reruns=rer, jac3_passes=0, rb4_passes=deep, pass_kind=1)
    return (conv if conv is not None and conv <= itr_max else itr_max + 1), dict(exact_reruns=0, jac3_passes=0, rb4_passes=0)


def switches(mode):
    """what the test forces before the solve (czhip_set_tuning2 enable, czhip_set_jac3 / czhip_set_rb4 enable)"""
    return {"single": dict(t2=0, jac3=0, rb4=0), "pair": dict(t2=1, jac3=0, rb4=0), "triple": dict(t2=1, jac3=2, rb4=0),
            "rb1": dict(t2=1, jac3=0, rb4=0), "rb4": dict(t2=1, jac3=0, rb4=2), "plain": dict(t2=1, jac3=1, rb4=1)}[mode]


def case(name, solver, prec, mode, gsz, coef, itr_max, conv, div=None, lag=None):
    it, cnt = counters(solver, mode, conv, itr_max)
    assert it == (conv if conv <= itr_max else itr_max + 1)
    c = dict(name=name, solver=solver, prec=prec, gsz=list(gsz), coef=coef, itr_max=itr_max, switches=switches(mode), mode=mode,
             converged_at=conv, iter=it, counters=cnt)
    if div is not None:
        c.update(div=list(div), lag_reduce=lag)
        c["counters"] = dict(exact_reruns=1, pass_kind=2, lagged_reduce=lag, buffers=3 if lag else 2)
    return c


def find(solver, prec, crange, pred, grids=GRIDS):
    for gsz in grids:
        for coef in coefs(*crange):
            conv, hist = oracle(gsz, solver, ITR_BIG, coef, prec)
            if conv <= ITR_BIG and pred(conv) and margin_ok(hist):
                return gsz, coef, conv
    raise RuntimeError(f"no landing found for {solver} {prec}")


def main():
    cases = []
    for name, solver, prec, mode, crange, pred in SEARCH:
        gsz, coef, conv = find(solver, prec, crange, pred)
        cases.append(case(name, solver, prec, mode, gsz, coef, ITR_BIG, conv))
    for name, mode, prec, delta, pred in ITRMAX:
        solver = "jacobi" if mode in ("pair", "triple") else "sor2sma"
        crange = (0.6, 1.0, 0.01) if solver == "jacobi" else (1.2, 1.9, 0.01)
        gsz, coef, conv = find(solver, prec, crange, pred)
        itr_max = conv + delta
        cases.append(case(name, solver, prec, mode, gsz, coef, itr_max, conv))
    for div, lag in DECOMP:
        gsz, coef, conv = find("jacobi", "f64", (0.6, 1.0, 0.01), lambda c: c % 2 == 1, grids=[(16, 16, 16), (20, 16, 16), (16, 20, 20)])
        cases.append(case(f"jacobi_decomposed_{'x'.join(map(str, div))}_lag{lag}_sweep1", "jacobi", "f64", "pair", gsz, coef, ITR_BIG, conv,
                          div=div, lag=lag))
    with open(OUT, "w") as f:
        json.dump(dict(eps=O.EPS, margin=MARGIN, poll_every=POLL_EVERY, cases=cases), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {OUT}")


if __name__ == "__main__":
    main()
