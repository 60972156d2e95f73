"""cz_bc.h without a GPU: the one description of the boundary faces -- a level's packed word and the fill's kinds from
it -- against the restatement of tests/periodic_parity.py, for every state and every level of 1, 2 or 5 points per direction."""
import itertools
import os
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neumann_parity as N  # noqa: E402
import periodic_parity as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lines(tmp_path):
    """tests/bc_words.cpp compiled with the host C++ compiler, its output"""
    exe = str(tmp_path / "bc_words")
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    cmd = [cxx] if cxx else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "c++"]
    cmd += ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cubez_amd", "csrc"), os.path.join(ROOT, "tests", "bc_words.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, "the state's constructors lost a flag"
    return r.stdout.splitlines()


def test_level_words_and_kinds_equal_the_restatement(tmp_path):
    want = []
    for nm, per in itertools.product(range(64), range(8)):
        faces, dirs = [(nm >> f) & 1 for f in range(6)], [(per >> d) & 1 for d in range(3)]
        for gn in itertools.product((1, 2, 5), repeat=3):
            f, w = P.level_state(gn, 0, faces, dirs)
            word = N.bits(f) | P.bits(w) << 6
            line = [nm, per, *gn, ":", word, ":", *P.kinds(f, w), ":", *P.kinds(N.NONE, w)]
            want.append(" ".join(map(str, line)))
    got = _lines(tmp_path)
    assert len(got) == len(want) == 64 * 8 * 27
    for g, w in zip(got, want):
        assert g == w
