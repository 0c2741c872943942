"""Pass times with and without an environment (hipEvents, one process).

    python scripts/env_time.py [--reps 20] [--only cornell|multi]

Configurations, each a fresh context, timed as the median over --reps warm passes between two events on the
stream (3 warm-up passes first), with the rays traced per pass from pt_stats (the sum of the live paths over
the bounces) and the share of paths that end in the first bounce:

  Cornell 800x800, depth 8, 16 iterations per pass (10.2 M paths):
      none        no environment (camera masks on)
      none_no_masks   the same without camera masks (PT_AMD_NO_CMASK=1), to tell their share of `zero`'s cost
      zero        an all-zero 8x8 map: the same paths and the same image, so the ratio to `none` is the cost of
                  the ENV instantiations plus the camera masks a context with an environment does not build
      map1024     a 1024^2 map (17 MB)
  the 4K multi-object scene of the benchmark's config 4, depth 8, 2 iterations per pass (16.6 M paths):
      none        no environment
      map2048     a 2048^2 map (67 MB)

The maps are a smooth generated sky (no file is read).  One JSON line per configuration; nothing is compared
with a threshold.  The ENV kernels' registers, scratch and occupancy are the compiler's, not
measured here; the map's share of the fabric traffic needs a counter run of its own and is not taken here.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import cuda_pathtracer_amd as P  # noqa: E402
from cuda_pathtracer_amd import scenes as S  # noqa: E402

LIB = os.path.basename(os.environ.get("PT_AMD_LIB", "libpt_amd.so"))


def sky(n):
    """A smooth (n, n, 3) octahedral map: brighter towards +y (the centre), a warm patch on one side."""
    c = (np.arange(n, dtype=np.float32) + 0.5) / n * 2 - 1
    z, x = np.meshgrid(c, c, indexing="ij")
    up = 1 - np.abs(x) - np.abs(z)
    base = 0.6 + 0.5 * up
    sun = np.exp(-((x - 0.35) ** 2 + (z + 0.2) ** 2) * 40.0)
    return np.stack([base + 6 * sun, base * 1.05 + 5 * sun, base * 1.2 + 3 * sun], -1).astype(np.float32)


def time_config(name, scene, label, spp, reps, torch):
    pt = P.PathTracer(scene, P.GuiDataContainer(), spp=spp)
    try:
        it = 1
        for _ in range(3):
            pt.render_pass(it)
            it += spp
        torch.cuda.synchronize()
        before = pt.stats()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            pt.render_pass(it)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
            it += spp
        torch.cuda.synchronize()
        after = pt.stats()
        live = [(x - y) / reps for x, y in zip(after["bounce_live"], before["bounce_live"])]
        rays = sum(live)
        med = statistics.median(ms)
        env = scene.environment()
        print(json.dumps({"what": "env_time", "lib": LIB, "scene": name, "config": label, "spp_per_pass": spp, "reps": reps,
                          "map_n": env["n"] if env else 0, "map_mbytes": round((env["n"] + 2) ** 2 * 16 / 1e6, 1) if env else 0,
                          "camera_masks": pt.cmask_info()["on"], "ms_per_pass": round(med, 4),
                          "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "rays_per_pass": int(rays),
                          "mray_per_s": round(rays / med / 1e3, 1),
                          "paths_ending_in_first_bounce": round(1 - live[1] / live[0], 4) if live[0] else None,
                          "image_mean": float(pt.image().mean())}), flush=True)
    finally:
        pt.free()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["cornell", "multi"], default=None)
    a = ap.parse_args(argv)
    import torch
    torch.cuda.set_device(0)
    if a.only in (None, "cornell"):
        scene = P.Scene(str(ROOT / "tests" / "scenes" / "cornell.json"))
        scene.set_camera((800, 800), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
        scene.set_render(1, 8)
        scene.finalize()
        time_config("cornell_800", scene, "none", 16, a.reps, torch)
        os.environ["PT_AMD_NO_CMASK"] = "1"              # (read when the context is created)
        time_config("cornell_800", scene, "none_no_masks", 16, a.reps, torch)
        del os.environ["PT_AMD_NO_CMASK"]
        scene.set_environment_octa(np.zeros((8, 8, 3), np.float32))
        time_config("cornell_800", scene, "zero", 16, a.reps, torch)
        scene.set_environment_octa(sky(1024))
        time_config("cornell_800", scene, "map1024", 16, a.reps, torch)
    if a.only in (None, "multi"):
        with tempfile.TemporaryDirectory() as tmp:
            scene = P.Scene(S.multi_object(tmp))
            time_config("multi_object_4k", scene, "none", 2, a.reps, torch)
            scene.set_environment_octa(sky(2048), rotate=(0.0, 30.0, 0.0))
            time_config("multi_object_4k", scene, "map2048", 2, a.reps, torch)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
