"""GPU: bench.py's plain run in a fresh process -- one JSON line with the headline keys and none of the --full objects, and
--dump-outputs writing the latents of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_latents(tmp_path):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    j = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert j["metric"] == "unet_denoise_steps_per_sec" and j["unit"] == "denoise_steps/s" and j["higher_is_better"] is True
    assert j["dtype"] == "bf16" and j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0
    assert abs(j["value"] * j["ms_per_step"] / 1e3 - 1.0) < 1e-2                 # value = steps / s = 1000 / ms_per_step
    assert not {"roofline", "floor", "k1", "train", "end_to_end", "fp8", "infer_b1", "cpu_baseline"} & set(j)
    lat = np.load(out / "latents.npy")
    assert lat.shape == (4, 8, 250, 16) and lat.dtype == np.float32 and np.isfinite(lat).all()
    sys.path.insert(0, ROOT)
    import bench
    noise = bench.synth_inputs(4, 250, 16)[0].numpy()
    assert np.abs(lat - noise).max() > 1e-3                                        # four DDIM steps moved the latents
