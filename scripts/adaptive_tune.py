"""The grid behind the adaptive-sampling defaults.

    python scripts/adaptive_tune.py [--out profiles/adaptive_tune.jsonl]

Cornell 200x200, rng_key_pixel on, batches of 4; reference = 1024 spp of the same setting; RMSE on values
clamped to [0, 1].  Budget B = the segments uniform 64 spp traces (pt_stats).  An adaptive run updates
after every batch, selects every 4 batches and stops once it has spent B segments or nothing is active
(so its last batch may take it past B: every line reports the segments spent beside the budget).
For every (threshold, floor, min_batches, dilate) of the grid: RMSE(adaptive) / RMSE(uniform 64 spp), raw
(resolved image against accumulator / 64) and after the variance-guided filter at its defaults on both.
The default minimises the raw ratio; the last line names the minimum and every setting within 0.1% of
it.  Prints one JSON line per setting before that.
"""
from __future__ import annotations

import argparse
import itertools
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import cuda_pathtracer_amd as P  # noqa: E402

THRESHOLDS = (0.05, 0.1, 0.2, 0.4, 0.6, 0.8)
FLOORS = (0.01, 0.1)
MIN_BATCHES = (4, 8)
DILATES = (0, 1, 2)
BATCH, EVERY, UNIFORM_SPP, REF_SPP = 4, 4, 64, 1024


def cornell(res=(200, 200)) -> "P.Scene":
    spec = json.loads((ROOT / "tests" / "scenes" / "cornell.json").read_text())
    spec["Camera"]["RES"] = list(res)
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "cornell.json"
        path.write_text(json.dumps(spec))
        return P.Scene(str(path))


def _gui():
    g = P.GuiDataContainer()
    g.rngKeyPixel = True
    return g


def rmse(img, ref) -> float:
    return float(np.sqrt(np.mean((np.clip(img, 0, 1).astype(np.float64) - ref) ** 2)))


def uniform(scene) -> dict:
    """Uniform 64 spp in batches of 4 with variance tracking, and the run continued to 1024 spp."""
    pt = P.PathTracer(scene, _gui(), spp=BATCH)
    pt.track_variance(True)
    out = {}
    for it in range(1, REF_SPP + 1, BATCH):
        pt.render_pass(it)
        n = it + BATCH - 1
        if n <= UNIFORM_SPP:
            pt.variance_update()
        if n == UNIFORM_SPP:
            out["raw"] = pt.image() / np.float32(n)
            out["filtered"] = pt.denoised_variance(float(n))
            out["segments"] = pt.stats()["segments"]
    out["ref"] = np.clip(pt.image() / np.float32(REF_SPP), 0, 1).astype(np.float64)
    pt.free()
    return out


def adaptive(scene, prm, budget: int, every: int = EVERY) -> dict:
    pt = P.PathTracer(scene, _gui(), spp=BATCH)
    pt.adaptive(True)
    active, batches, seg = [], 0, 0
    for it in range(1, REF_SPP + 1, BATCH):
        pt.render_pass(it)
        pt.adaptive_update()
        batches += 1
        seg = pt.stats()["segments"]
        if seg >= budget:
            break
        if batches % every == 0:
            active.append(pt.adaptive_select(prm)["active_blocks"])
            if active[-1] == 0:
                break
    nb = pt.adaptive_state()["nb"]
    out = {"raw": pt.adaptive_image(), "filtered": pt.adaptive_image(P.DenoiseVarParams.default()), "segments": seg,
           "batches": batches, "active": active, "blocks": int(nb.size), "nb_min": int(nb.min()), "nb_max": int(nb.max()),
           "nb_mean": float(nb.mean())}
    pt.free()
    return out


def params(threshold, floor, min_batches, dilate):
    p = P.AdaptiveParams.default()
    p.threshold, p.floor, p.min_batches, p.dilate = threshold, floor, min_batches, dilate
    return p


def ratios(scene, uni, prm) -> dict:
    a = adaptive(scene, prm, uni["segments"])
    return {"raw_ratio": rmse(a["raw"], uni["ref"]) / rmse(uni["raw"], uni["ref"]),
            "filtered_ratio": rmse(a["filtered"], uni["ref"]) / rmse(uni["filtered"], uni["ref"]),
            "segments": a["segments"], "budget": uni["segments"], "batches": a["batches"], "active": a["active"],
            "blocks": a["blocks"], "nb_min": a["nb_min"], "nb_max": a["nb_max"], "nb_mean": round(a["nb_mean"], 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    scene = cornell()
    uni = uniform(scene)
    lines = [{"uniform_rmse_raw": rmse(uni["raw"], uni["ref"]), "uniform_rmse_filtered": rmse(uni["filtered"], uni["ref"]),
              "budget_segments": uni["segments"]}]
    rows = []
    for t, f, m, d in itertools.product(THRESHOLDS, FLOORS, MIN_BATCHES, DILATES):
        rows.append({"threshold": t, "floor": f, "min_batches": m, "dilate": d, **ratios(scene, uni, params(t, f, m, d))})
    lines += rows
    best = min(r["raw_ratio"] for r in rows)
    lines.append({"min_raw_ratio": best,
                  "within_0.1_percent": [[r["threshold"], r["floor"], r["min_batches"], r["dilate"]] for r in rows
                                         if r["raw_ratio"] <= best * 1.001]})
    text = "\n".join(json.dumps(r) for r in lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
