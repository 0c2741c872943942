"""The grid behind the variance-guided filter's default sigma_l.

    python scripts/denoise_var_tune.py

Cornell 200x200, a spp = 4 context tracking the variance (batches of 4), reference = 1024 spp of the same
run.  At 16, 64 and 256 spp: the RMSE (values clamped to [0, 1]) of the raw image, of the plain filter at
its defaults and of the variance-guided filter for sigma_l in {0.5, 1, 2, 4, 8} (sigma_n, sigma_p and the
levels at their defaults).  The score of a sigma_l is the sum of its RMSE ratios to raw at 16 and 256 spp.
Prints one JSON line per sample count and one with the scores.
"""
from __future__ import annotations

import json
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import cuda_pathtracer_amd as P  # noqa: E402

SIGMAS = (0.5, 1.0, 2.0, 4.0, 8.0)
COUNTS = (16, 64, 256)


def main() -> int:
    spec = json.loads((ROOT / "tests" / "scenes" / "cornell.json").read_text())
    spec["Camera"]["RES"] = [200, 200]
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "cornell.json"
        path.write_text(json.dumps(spec))
        scene = P.Scene(str(path))
    pt = P.PathTracer(scene, spp=4)
    pt.track_variance(True)
    g = pt.gbuffer()
    shots = {}
    for it in range(1, 1025, 4):
        pt.render_pass(it)
        n = it + 3
        if n <= max(COUNTS):
            pt.variance_update()
        if n in COUNTS:
            shots[n] = (pt.image(), pt.variance(float(n)), pt.denoised(float(n)))
    ref = np.clip(pt.image() / np.float32(1024), 0, 1).astype(np.float64)
    pt.free()

    def rmse(a):
        return float(np.sqrt(np.mean((np.clip(a, 0, 1).astype(np.float64) - ref) ** 2)))

    ratios = {s: {} for s in SIGMAS}
    for n, (img, var, plain) in shots.items():
        raw = rmse(img / np.float32(n))
        row = {"spp": n, "raw": round(raw, 5), "plain": round(rmse(plain), 5), "variance_guided": {},
               "median_variance": float(np.median(var))}
        for s in SIGMAS:
            prm = P.DenoiseVarParams.default()
            prm.sigma_l = s
            r = rmse(P.denoise_variance(img, float(n), var, g, prm))
            row["variance_guided"][str(s)] = round(r, 5)
            ratios[s][n] = r / raw
        print(json.dumps(row), flush=True)
    score = {str(s): round(ratios[s][16] + ratios[s][256], 4) for s in SIGMAS}
    print(json.dumps({"score_ratio16_plus_ratio256": score, "best_sigma_l": min(score, key=score.get)}), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
