"""bench.py on one GPU, as the driver runs it: a plain run measures the headline and nothing else (the objects that need
runs of their own are null), `--full` adds the host/GPU balance, the per-kernel stage times and the roofline."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 20000


def _run_bench(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2",
           "--init-steps", "4", "--init-seconds", "0", "--points", str(P)] + extra
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def _check_headline(line):
    assert line["metric"] == "rasterize fwd+bwd Gaussians/sec @1024^2, 100k pts"
    assert line["unit"] == "Gaussians/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["n_gpus"] == 1 and line["steps"] == 6 and line["warmup"] == 2
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert abs(line["value"] - P * 1e3 / line["ms_per_step"]) <= 1e-6 * line["value"]     # value = P * K / t
    assert line["config"]["num_rendered_R"] > 0


@pytest.mark.timeout(900)
def test_plain_run_measures_the_headline_only():
    line = _run_bench([])
    _check_headline(line)
    for k in ("host", "stage_us", "roofline", "cpu_baseline", "extra", "collective"):
        assert line[k] is None, k


@pytest.mark.timeout(900)
def test_full_run_adds_host_stage_times_and_roofline():
    line = _run_bench(["--full", "--no-cpu-baseline", "--no-extra"])
    _check_headline(line)
    assert line["host"]["step_us"] > 0 and line["host"]["forward_calls_total"] > 0
    assert set(line["stage_us"]) == {"preprocess_fwd", "tiles", "fill", "sort", "render_fwd", "render_bwd", "pair_reduce",
                                     "preprocess_bwd"}
    assert all(v >= 0 for v in line["stage_us"].values()) and sum(line["stage_us"].values()) > 0
    r = line["roofline"]
    assert r["kernel"] in ("preprocess_fwd", "tiles", "fill", "sort", "render_fwd", "blend_bwd(render_bwd+pair_reduce)",
                           "preprocess_bwd")
    assert r["achieved"] > 0 and r["avg_us"] > 0 and r["path"]["ms_per_step"] == line["ms_per_step"]
    assert line["cpu_baseline"] is None and line["extra"] is None          # skipped on request
