"""GPU test (-m gpu): the name matrix of the `cz` command line.  tests/golden/cli_matrix.json (tests/golden/make_cli_matrix.py) holds, for
every solver name, every preconditioner name of pbicgstab, pbicgstab_maf and pcg, a few names in another letter case and the refusals, what
the command line printed, wrote and returned before the names were gathered into one table (cubez_amd/csrc/cz_solvers.h).  Every run is
deterministic run to run, so each recorded item must come out equal: a row of the table that states anything else than
the branch it replaced -- role, MAF flag, loop, copy or solve as a preconditioner, a line solver's order or final stage -- changes one."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = json.load(open(os.path.join(GOLDEN, "cli_matrix.json")))

_spec = importlib.util.spec_from_file_location("make_cli_matrix", os.path.join(GOLDEN, "make_cli_matrix.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

_signalled = []   # the first run that a signal or the time limit ended: nothing is started on the GPU after it


def test_the_fixture_holds_every_name():
    """both precisions; every solver alone, every preconditioner of every Krylov solver, the refusals"""
    recorded = {(c["prec"], tuple(c["args"])) for c in CASES}
    wanted = {(p, tuple(str(a) for a in args)) for p in ("f32", "f64") for args in gen.command_lines()}
    assert recorded == wanted and len(CASES) == len(wanted)
    pre = {(c["args"][3], c["args"][6]) for c in CASES if len(c["args"]) > 6 and "lines" in c}
    assert len({p for s, p in pre if s == "pbicgstab"}) == 16 and {p for s, p in pre if s == "pcg"} >= {"none", "jacobi", "mg", "mgrb"}
    assert sum(1 for c in CASES if "stdout" in c) == 2 * 6   # pbicgstab and pbicgstab_maf alone, and the four refused names


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join([c["prec"]] + c["args"][3:4] + c["args"][6:]))
def test_cli_run_equals_the_recorded_one(case):
    if _signalled:
        pytest.fail(f"not run: {_signalled[0]} was ended by a signal or the time limit")
    got = gen.run(case["prec"], case["args"])   # one run, under its own time limit
    if got is None:
        _signalled.append(" ".join(case["args"]))
        pytest.fail("ended by a signal or the time limit")
    for key in sorted(set(case) | set(got)):
        assert got.get(key) == case.get(key), key
