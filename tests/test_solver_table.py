"""CPU-side checks that a solver's or preconditioner's name is stated once: cubez_amd/csrc/cz_solvers.h holds one row per name, and the
driver and the command line look names up there instead of restating them (no GPU needed; the usage text is printed before HIP starts)."""
import os
import re
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "cubez_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _code(name):
    """a source file without its // comments"""
    return "\n".join(ln.split("//")[0] for ln in open(os.path.join(SRC, name)).read().splitlines())


def test_names_are_matched_in_one_place_and_ids_are_not_compared_by_order():
    for name in ("cz_driver.cpp", "cz_main.cpp"):
        src = _code(name)
        assert "strcasecmp(" not in src, name            # name matching lives in cz_solvers.h
        assert not re.search(r"[<>]=?\s*LS_", src), name   # no enum-range test: the next inserted enumerator would break it silently
    assert "strcasecmp(" in _code("cz_solvers.h")


def test_solver_names_are_spelled_in_one_file():
    """the names that are neither section-timing labels nor parts of a message occur, as quoted literals, in cz_solvers.h alone"""
    for name in ("pcr_rb_esa_maf", "pcr_eda_maf", "pcr_j_esa", "pbicgstab_maf", "sor2sma_maf", "psor_maf"):
        files = sorted(f for f in os.listdir(SRC) if os.path.isfile(os.path.join(SRC, f)) and f'"{name}"' in open(os.path.join(SRC, f), errors="replace").read())
        assert files == ["cz_solvers.h"], (name, files)


def test_the_enum_keeps_the_reference_values():
    """cz_Define.h:68-89 numbers the solvers; the table's rows are found by id, so the values may stay what they were"""
    body = re.search(r"enum LinearSolver \{(.*?)\}", _code("cz_solvers.h"), re.S).group(1)
    val, got = -1, {}
    for item in body.split(","):
        k, _, v = (t.strip() for t in item.partition("="))
        val = int(v) if v else val + 1
        got[k] = val
    assert got == dict(LS_NONE=0, LS_PSOR=1, LS_SOR2SMA=2, LS_BICGSTAB=3, LS_JACOBI=4, LS_PCR=5, LS_PCR_EDA=6, LS_PCR_ESA=7, LS_PCR_RB=8,
                       LS_PCR_RB_ESA=9, LS_PCR_J_ESA=10, LS_PSOR_MAF=11, LS_SOR2SMA_MAF=12, LS_BICGSTAB_MAF=13, LS_JACOBI_MAF=14, LS_PCR_MAF=15,
                       LS_PCR_EDA_MAF=16, LS_PCR_ESA_MAF=17, LS_PCR_RB_MAF=18, LS_PCR_RB_ESA_MAF=19, LS_PCG=20, LS_MG=21, LS_MGRB=22)
    rows = re.findall(r"^\s*\{(LS_[A-Z0-9_]+), \"", _code("cz_solvers.h"), re.M)
    assert sorted(rows) == sorted(got) and len(set(rows)) == len(rows)   # one row per enumerator


def test_usage_text_is_the_recorded_one():
    """cz with a wrong argument count prints the usage and returns before the GPU is touched; both name lists come from the table and must
    equal, byte for byte, what the command line printed when they were literals (tests/golden/cli_usage.txt)"""
    for prec in ("f32", "f64"):
        exe = os.path.join(ROOT, "cubez_amd", f"cz_{prec}")
        assert os.path.exists(exe), "build the command line: make -C cubez_amd/csrc"
        r = subprocess.run([exe, "24", "20", "28"], capture_output=True, timeout=120, env={k: v for k, v in os.environ.items() if k != "RANK"})
        assert r.returncode == 0 and r.stdout == open(os.path.join(GOLDEN, "cli_usage.txt"), "rb").read()
