"""The grid behind the temporal history's default min_ndot, plane_tol and max_history.

    python scripts/temporal_tune.py [--steps 8]

Cornell 200x200, world == 1, spp = 1 contexts.  A sequence is 16 samples at the loaded camera, then
--steps orbit steps in phi of 1 sample each (a new context per step, as the preview restarts), for step
sizes of 1, 4 and 16 pixels' worth of phi (k / width: the size of real mouse events).  The reference of
each view is 1024 spp of that view.  Each sequence is rendered once (accumulators, G-buffers and cameras
kept on the host) and replayed through TemporalHistory.frame_arrays for every parameter set.  Per moved
view: the RMSE (values clamped to [0, 1]) of the raw 1 spp image, of the plain filter on it (§10's
defaults), of the history's resolved mean, and of the variance-guided filter on the history (§11's
defaults).  The score of a parameter set is the sum over the step sizes of the mean ratio
RMSE(temporal + variance-guided) / RMSE(raw); the tie rule is in main().  Prints one JSON line per
(parameter set, step size), one with the scores, and one per step size at the chosen set, split into
reflective first hits (the history ghosts there) and the rest where the scene has any.
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

RES = 200
STEP_PIXELS = (1, 4, 16)
MIN_NDOT = (0.5, 0.9, 0.99)
PLANE_TOL = (0.005, 0.02, 0.1)
MAX_HISTORY = (8.0, 32.0, 0.0)


def record(path, step_pixels, steps):
    """One sequence: a list of (camera, [accumulator after each pass], gbuffer, reference or None)."""
    scene = P.Scene(path)
    phi, theta, zoom = scene.orbit()
    look = list(scene.camera().look_at[:3])
    views = []
    for k in range(steps + 1):
        if k:
            scene.set_orbit(phi - k * step_pixels / RES, theta, zoom, look)
        pt = P.PathTracer(scene)
        accs = []
        for it in range(1, (16 if k == 0 else 1) + 1):
            pt.render_pass(it)
            accs.append(pt.image())
        g = pt.gbuffer()
        pt.free()
        ref = None
        if k:
            big = P.PathTracer(scene, spp=256)
            for it in range(1, 1025, 256):
                big.render_pass(it)
            ref = np.clip(big.image() / np.float32(1024), 0, 1).astype(np.float64)
            big.free()
        views.append((scene.camera(), accs, g, ref))
    return views


def rmse(a, ref, mask=None):
    d = (np.clip(a, 0, 1).astype(np.float64) - ref) ** 2
    return float(np.sqrt(np.mean(d if mask is None else d[mask])))


def replay(views, prm, split=False):
    """Mean RMSE over the moved views of raw, plain, temporal and temporal + variance-guided."""
    hist = P.TemporalHistory(RES, RES, prm)
    rows = []
    for cam, accs, g, ref in views:
        for n, acc in enumerate(accs, 1):
            hist.frame_arrays(cam, acc, float(n), g)
        if ref is None:
            continue
        raw = accs[-1]
        imgs = {"raw": raw, "plain": P.denoise(raw, 1.0, g), "temporal": hist.image(),
                "temporal_var": hist.image(P.DenoiseVarParams.default())}
        row = {k: rmse(v, ref) for k, v in imgs.items()}
        if split:   # the mirror sphere (reflective first hits: the history ghosts there) and the rest
            mats = SCENE.materials()
            refl = np.array([m.has_reflective > 0 for m in mats])
            on = (g["mat"] >= 0) & refl[np.maximum(g["mat"], 0)]
            row["reflective_first_hits"] = float(on.mean())
            for k, v in imgs.items() if on.any() else ():
                row[k + "_reflective"] = rmse(v, ref, on)
                row[k + "_rest"] = rmse(v, ref, ~on)
        row["kept"] = float((hist.image(return_history=True)[1] > 1).mean())
        rows.append(row)
    hist.free()
    return {k: float(np.mean([r[k] for r in rows])) for k in rows[0]}


SCENE = None


def main(argv=None) -> int:
    global SCENE
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=8)
    a = ap.parse_args(argv)
    spec = json.loads((ROOT / "tests" / "scenes" / "cornell.json").read_text())
    spec["Camera"]["RES"] = [RES, RES]
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "cornell.json"
        path.write_text(json.dumps(spec))
        SCENE = P.Scene(str(path))
        seqs = {s: record(str(path), s, a.steps) for s in STEP_PIXELS}
    scores = {}
    for nd, tol, mh in itertools.product(MIN_NDOT, PLANE_TOL, MAX_HISTORY):
        prm = P.TemporalParams.default()
        prm.min_ndot, prm.plane_tol, prm.max_history = nd, tol, mh
        key = f"{nd}/{tol}/{mh}"
        scores[key] = 0.0
        for s in STEP_PIXELS:
            row = replay(seqs[s], prm)
            scores[key] += row["temporal_var"] / row["raw"]
            print(json.dumps({"min_ndot": nd, "plane_tol": tol, "max_history": mh, "step_pixels": s, "steps": a.steps,
                              **{k: round(v, 5) for k, v in row.items()}}), flush=True)
    # Sets within 0.001 of the lowest score are tied.  Among them: the strictest normal test, then the
    # shortest bounded history (a bound ages out what the guides cannot see), then the plane tolerance
    # in the middle of its tied values (no extreme of a range that made no difference).
    low = min(scores.values())
    tied = [tuple(float(v) for v in k.split("/")) for k, v in scores.items() if v <= low + 1e-3]
    nd = max(t[0] for t in tied)
    tied = [t for t in tied if t[0] == nd]
    mh = min((t[2] for t in tied if t[2] > 0), default=0.0)
    tols = sorted(t[1] for t in tied if t[2] == mh)
    best = f"{nd}/{tols[len(tols) // 2]}/{mh}"
    print(json.dumps({"score_sum_of_ratios_to_raw": {k: round(v, 4) for k, v in scores.items()}, "lowest": round(low, 4),
                      "tied": len([v for v in scores.values() if v <= low + 1e-3]), "best": best}), flush=True)
    nd, tol, mh = (float(v) for v in best.split("/"))
    prm = P.TemporalParams.default()
    prm.min_ndot, prm.plane_tol, prm.max_history = nd, tol, mh
    for s in STEP_PIXELS:
        row = replay(seqs[s], prm, split=True)
        print(json.dumps({"best": best, "step_pixels": s, "split": True, **{k: round(v, 5) for k, v in row.items()}}), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
