"""GPU test (-m gpu) of `bench.py --dump-outputs DIR`: what the timed path computed in its last step, written as .npy files, the same from
run to run (the settle sweeps run on a second instance, so the timed steps start from the set-up state), and -- for the Jacobi headline --
the oracle's field after exactly warm-up + repeats x steps sweeps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cz_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS, WARMUP, REPEATS = 64, 7, 2, 2
LEGS = {"jacobi_f32": np.float32, "sor2sma_f32": np.float32, "pbicgstab_f64": np.float64}


def _bench(out_dir):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", str(N), "--steps", str(STEPS), "--warmup", str(WARMUP),
                        "--repeats", str(REPEATS), "--no-cpu-baseline", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dump_outputs_are_reproducible_and_what_the_timed_path_computed(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    line = _bench(a)
    _bench(b)
    assert line["steps"] == STEPS and line["ms_per_step"] > 0 and "error" not in line["configs"], line
    names = sorted(os.listdir(a))
    assert names == sorted(f"{leg}_{x}.npy" for leg in LEGS for x in ("P", "residual_history", "residual"))
    assert names == sorted(os.listdir(b))
    assert sum(os.path.getsize(a / f) for f in names) <= 64 << 20
    for f in names:
        assert (a / f).read_bytes() == (b / f).read_bytes(), f"{f} differs between two runs with the same arguments"
    for leg, real in LEGS.items():
        P, hist = np.load(a / f"{leg}_P.npy"), np.load(a / f"{leg}_residual_history.npy")
        assert P.dtype == real and P.shape == (N, N, N)
        assert hist.dtype == np.float64 and len(hist) == (min(STEPS, 10) if leg.startswith("pbicgstab") else STEPS)
        assert np.load(a / f"{leg}_residual.npy")[0] == hist[-1]
    # the Jacobi leg: set-up state, WARMUP + REPEATS x STEPS sweeps, nothing else
    o = O.run((N, N, N), "jacobi", WARMUP + REPEATS * STEPS, 0.8, kind="oracle", prec="f32", wide=True)
    g = 2
    assert np.load(a / "jacobi_f32_P.npy").tobytes() == np.ascontiguousarray(o.P[g:-g, g:-g, g:-g]).tobytes()
