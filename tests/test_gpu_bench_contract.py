"""The driver's bench contract: `python bench.py --gpus 1 --steps K --warmup W` prints ONE JSON line with the agreed
keys; `--full` adds the parity leg, the roofline and the CPU baseline; `--dump-outputs DIR` writes what the timed steps
computed.  Runs a reduced scene (`--pts`, which the bench itself labels as debug-only) in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *argv], capture_output=True, text=True, timeout=280,
                         env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bench_json_contract(hip):
    d = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--pts", "3000", "--full")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    r = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    c = d["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in c, key
    assert c["kind"] in ("port", "reference") and c["value"] > 0
    assert d["rmse_px"]["rel_diff_gpu_vs_cpu"] < 1e-9          # the parity leg of the bench itself


def test_plain_bench_times_k_steps_and_dumps_their_result(hip, sfm, oracle, tmp_path):
    """Without --full: one timed region of exactly K steps, no CPU leg; the dumped state is K iterations from the
    scene's initial estimate, i.e. the oracle's result for the same scene and iteration count."""
    d = _bench("--gpus", "1", "--steps", "3", "--warmup", "2", "--pts", "3000", "--dump-outputs", str(tmp_path))
    for key in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "dtype"):
        assert key in d, key
    assert d["steps"] == 3 and d["warmup"] == 2 and d["repeats"] == 1 and len(d["ms_per_step_runs"]) == 1
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert d["higher_is_better"] is True and d["dtype"] == "f64"
    assert "cpu_baseline" not in d and "roofline" not in d
    cams, pts = np.load(tmp_path / "cams.npy"), np.load(tmp_path / "pts.npy")
    assert cams.dtype == np.float64 and pts.dtype == np.float64 and cams.shape == (50, 7) and pts.shape == (3, 3000)
    cfg = sfm.scenes.CONFIGS["C3"]
    sc = sfm.scenes.make_scene(cfg["n_cams"], 3000, cfg["visibility"], seed=0)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    ocams, opts = oracle.ba_sparse(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, 5.0, 3)
    assert np.max(np.abs(cams - ocams)) / np.max(np.abs(ocams)) < 1e-9
    assert np.max(np.abs(pts - opts)) / np.max(np.abs(opts)) < 1e-9
