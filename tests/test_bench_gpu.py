"""bench.py end to end on the GPU: a plain run times the steps it is asked for and prints the result
line without the side legs; --dump-outputs writes the framebuffer of the last timed step, which is
the accumulator the same passes leave in a PathTracer of this process, bit for bit."""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.gpu


def test_plain_run_is_lean_and_dumps_the_last_steps_image(cornell_path, gpu_device, tmp_path):
    steps, warmup = 2, 1
    out = tmp_path / "dump"
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                          str(warmup), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120,
                         cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line["unit"] == "Mray/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == steps and line["warmup"] == warmup and line["full"] is False
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region: segments / (steps x ms_per_step)
    assert line["value"] == pytest.approx(line["segments"] / (steps * line["ms_per_step"] * 1e-3) / 1e6, rel=1e-9)
    # the side legs stay behind --full
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert not {"scan", "compact", "dropin", "cpu_baseline_mt"} & set(line)
    assert sorted(p.name for p in out.iterdir()) == ["bounce_live.npy", "image.npy"]
    img, live = np.load(out / "image.npy"), np.load(out / "bounce_live.npy")
    assert img.dtype == np.float32 and img.shape == (800, 800, 3) and live.dtype == np.float64

    # the same passes here: iterations 1 .. (warmup + steps) x 256, one pass of 256 per step
    import torch
    import cuda_pathtracer_amd as P
    spp = line["config"]["iterations_per_pass"]
    assert spp == 256 and line["config"]["passes_per_step"] == 1
    pt = P.PathTracer(P.Scene(cornell_path), P.GuiDataContainer(), spp=spp)
    for k in range(warmup):
        pt.render_pass(1 + k * spp)
    torch.cuda.synchronize()
    s0 = pt.stats()
    for k in range(warmup, warmup + steps):
        pt.render_pass(1 + k * spp)
    want, s1 = pt.image(), pt.stats()
    pt.free()
    assert img.tobytes() == want.tobytes(), "the dumped image is not the accumulator after the last timed step"
    assert live.tolist() == [float(b - a) for a, b in zip(s0["bounce_live"], s1["bounce_live"])]
    assert line["bounce_live_per_step"] == [x / steps for x in live.tolist()]
