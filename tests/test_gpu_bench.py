"""bench.py on the GPU: a plain run (no --full) prints the headline line only and, with
--dump-outputs, writes what its last timed step computed.  One small run of the real benchmark
process (1024 rays, T = 2^16), shared by the tests."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")
N_RAYS, STEPS, WARMUP = 1024, 4, 2
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "grid_bw_ms", "eager_stage_ms", "density_update_ms", "value_with_occupancy_refresh",
             "cpu_baseline")


@pytest.fixture(scope="module")
def plain_run(gpu, tmp_path_factory):
    out = tmp_path_factory.mktemp("bench") / "outputs"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                        "--n-rays", str(N_RAYS), "--log2-T", "16", "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), out


@pytest.mark.gpu
def test_plain_line_holds_the_headline_only(plain_run):
    d, _ = plain_run
    for k in HEADLINE:
        assert k in d, k
    assert d["full"] is False
    for k in FULL_ONLY:
        assert k not in d, k
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["n_gpus"] == 1
    assert d["unit"] == "rays/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0
    # value = rays of the timed steps / their time; ms_per_step = that time / steps (both rounded)
    assert d["value"] == pytest.approx(N_RAYS / (d["ms_per_step"] * 1e-3), rel=1e-2)


@pytest.mark.gpu
def test_dumped_outputs_are_the_last_steps(plain_run):
    _, out = plain_run
    a = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(a) == {"batch", "rgb", "opacity", "depth", "samples_per_ray", "loss", "params_mlp", "params_table"}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k, v in a.items():
        assert v.dtype in (np.float32, np.float64), k
        assert np.isfinite(v).all(), k
    assert a["batch"].shape == (3, N_RAYS, 3)
    assert a["rgb"].shape == (N_RAYS, 3) and a["opacity"].shape == (N_RAYS,) and a["depth"].shape == (N_RAYS,)
    assert a["samples_per_ray"].shape == (N_RAYS,) and a["samples_per_ray"].sum() > 0
    assert a["loss"].shape == (1,) and a["loss"][0] > 0
    assert (a["opacity"] >= 0).all() and (a["opacity"] <= 1 + 1e-5).all()
    # the parameters were trained: the table no longer holds only its U(-1e-4, 1e-4) initial values
    assert np.abs(a["params_table"]).max() > 1e-4
    assert a["params_mlp"].size > 3072
