#!/usr/bin/env python3
"""Generate cli_matrix.json and cli_usage.txt: what the `cz` command line (cubez_amd/cz_f32, cz_f64) prints, writes and returns for
every solver and preconditioner name it accepts, and for the names it refuses.

One small anisotropic box, a fixed small ItrMax, both precisions:
  * every linear_solver name alone (pbicgstab and pbicgstab_maf alone are refusals: "command line error : pbicgstab");
  * pbicgstab with `none` and each of its 15 preconditioner names; pbicgstab_maf with none, jacobi, jacobi_maf, sor2sma_maf, pcr_rb_maf;
  * pcg with none, jacobi, mg, mgrb;
  * names in another letter case (matching is case-insensitive, the history file's name is lower case);
  * the refusals: an unknown solver, pbicgstab with mg / pcr_esa, pcg with sor2sma.
Recorded per run: the exit code; the stdout lines "Iterative Mehtod = ", "Preconditioner = ", "Iter = .. Res = ..", "Error max = .."
verbatim; the name of the history file and its sha256; the solver's name in profiling.txt's last line.  For a refusal: the whole stdout
and the files left behind.  Every run is deterministic run to run, so tests/test_gpu_cli_matrix.py asks for equality.  Needs a GPU and
the built command line (make -C cubez_amd/csrc).

    python tests/golden/make_cli_matrix.py [output directory, default tests/golden]
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
GSZ = [24, 20, 28]
ITR_MAX = 20
TIMEOUT = 120   # seconds per run
KEEP = ("Iterative Mehtod = ", "Preconditioner = ", "Iter = ", "Error max = ")

SOLVERS = ["jacobi", "psor", "sor2sma", "pbicgstab", "pcr", "pcr_eda", "pcr_esa", "pcr_rb", "pcr_rb_esa", "pcr_j_esa", "jacobi_maf", "psor_maf",
           "sor2sma_maf", "pbicgstab_maf", "pcr_maf", "pcr_eda_maf", "pcr_esa_maf", "pcr_rb_maf", "pcr_rb_esa_maf", "pcg"]
PBICGSTAB_PRE = ["none", "jacobi", "psor", "sor2sma", "pcr", "pcr_eda", "pcr_rb", "pcr_rb_esa", "pcr_j_esa", "jacobi_maf", "psor_maf",
                 "sor2sma_maf", "pcr_maf", "pcr_eda_maf", "pcr_rb_maf", "pcr_rb_esa_maf"]
PBICGSTAB_MAF_PRE = ["none", "jacobi", "jacobi_maf", "sor2sma_maf", "pcr_rb_maf"]
PCG_PRE = ["none", "jacobi", "mg", "mgrb"]
OTHER_CASE = [("Jacobi", None), ("PCR_RB_MAF", None), ("PBiCGSTAB", "SOR2SMA"), ("pcg", "MG")]
REFUSED = [("lsor_simd", None), ("pbicgstab", "mg"), ("pbicgstab", "pcr_esa"), ("pcg", "sor2sma")]


def coef(solver):
    """relaxed Jacobi sweeps (alone, or inside pbicgstab and pcg) below one, the SOR family above"""
    s = solver.lower()
    return 0.8 if s.startswith(("jacobi", "pbicgstab", "pcg")) else 1.1


def command_lines():
    pairs = [(s, None) for s in SOLVERS]
    pairs += [("pbicgstab", p) for p in PBICGSTAB_PRE] + [("pbicgstab_maf", p) for p in PBICGSTAB_MAF_PRE] + [("pcg", p) for p in PCG_PRE]
    pairs += OTHER_CASE + REFUSED
    return [GSZ + [s, ITR_MAX, coef(s)] + ([p] if p else []) for s, p in pairs]


def run(prec, args):
    """one run of the command line in an empty directory -> the recorded items (None: the process was ended by a signal or the time limit)"""
    exe = os.path.join(ROOT, "cubez_amd", f"cz_{prec}")
    assert os.path.exists(exe), "build the command line: make -C cubez_amd/csrc"
    with tempfile.TemporaryDirectory() as d:
        try:
            r = subprocess.run([exe] + [str(a) for a in args], cwd=d, capture_output=True, text=True, timeout=TIMEOUT)
        except subprocess.TimeoutExpired:
            return None
        if r.returncode < 0:
            return None
        rec = dict(prec=prec, args=[str(a) for a in args], exit=r.returncode)
        files = sorted(os.listdir(d))
        hist = [f for f in files if f.endswith(".txt") and f != "profiling.txt"]
        if "Iter = " not in r.stdout:   # a refusal: nothing was solved
            rec.update(stdout=r.stdout, files=files)
            return rec
        rec["lines"] = [ln for ln in r.stdout.splitlines() if ln.startswith(KEEP)]
        assert len(hist) == 1, files
        rec["history_file"] = hist[0]
        rec["history_sha256"] = hashlib.sha256(open(os.path.join(d, hist[0]), "rb").read()).hexdigest()
        m = re.search(r"Inclusive section: (\S+) ", open(os.path.join(d, "profiling.txt")).read())
        rec["profile_section"] = m.group(1) if m else None
        return rec


def usage(prec="f32"):
    exe = os.path.join(ROOT, "cubez_amd", f"cz_{prec}")
    return subprocess.run([exe] + [str(a) for a in GSZ], capture_output=True, text=True, timeout=TIMEOUT).stdout


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else HERE
    os.makedirs(out, exist_ok=True)
    cases = []
    for prec in ("f32", "f64"):
        for args in command_lines():
            rec = run(prec, args)
            if rec is None:
                sys.exit(f"cz_{prec} {args}: ended by a signal or the time limit; nothing written")
            cases.append(rec)
            print(prec, " ".join(rec["args"][3:]), "->", rec.get("lines", rec.get("stdout")), flush=True)
    with open(os.path.join(out, "cli_matrix.json"), "w") as f:
        json.dump(cases, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(os.path.join(out, "cli_usage.txt"), "w") as f:
        f.write(usage())
    print(f"{len(cases)} runs -> {out}")


if __name__ == "__main__":
    main()
