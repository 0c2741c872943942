"""Pass time against the share of active blocks, one process.

    python scripts/adaptive_pass_time.py [--spp 16] [--passes 8] [--reps 5]

Cornell 800x800, the fused pipeline, an adaptive context with explicit masks at 100 / 50 / 25 / 0 % of its
10,000 blocks, as random blocks and as one contiguous run of blocks from the top of the image.  A
measurement is the wall time of --passes passes of --spp iterations between two context synchronisations
(pt_stats), per pass; the settings alternate within every repetition and the figure is the median over
--reps of them, relative to the 100 % mask of the same repetition loop.  PT_AMD_SKIP_EMPTY = 0 / 1 forces
the first bounce's plain / empty-wave instantiation; unset, the context chooses from the effective masks'
empty share (>= 0.2: empty-wave).  Shows what an inactive block still costs in the first bounce.  Prints
one JSON line per (skip, kind, share).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import cuda_pathtracer_amd as P  # noqa: E402

SHARES = (1.0, 0.5, 0.25, 0.0)


def masks(nblk):
    rng = np.random.default_rng(2)
    order = rng.permutation(nblk)
    out = {}
    for s in SHARES:
        n = int(round(s * nblk))
        r = np.zeros(nblk, np.uint8)
        r[order[:n]] = 1
        c = np.zeros(nblk, np.uint8)
        c[:n] = 1
        out[("random", s)] = r
        out[("contiguous", s)] = c
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args(argv)
    scene = P.Scene(str(ROOT / "tests" / "scenes" / "cornell.json"))
    for skip in ("0", "1", None):
        if skip is None:
            os.environ.pop("PT_AMD_SKIP_EMPTY", None)
        else:
            os.environ["PT_AMD_SKIP_EMPTY"] = skip
        pt = P.PathTracer(scene, spp=a.spp)
        pt.adaptive(True)
        ms = masks((pt.npix + 63) // 64)
        times = {k: [] for k in ms}
        live1 = {}
        it = 1
        for rep in range(a.reps + 1):
            for key, m in ms.items():
                pt.adaptive_set_mask(m)
                s0 = pt.stats()
                t0 = time.perf_counter()
                for _ in range(a.passes):
                    pt.render_pass(it)
                    it += a.spp
                s1 = pt.stats()
                if rep:   # (the first repetition warms up)
                    times[key].append((time.perf_counter() - t0) * 1e3 / a.passes)
                live1[key] = (s1["bounce_live"][1] - s0["bounce_live"][1]) / a.passes
                used = pt.cmask_info()["skip_fused"]
                live1[(key, "skip")] = used
        base = {kind: statistics.median(times[(kind, 1.0)]) for kind in ("random", "contiguous")}
        for (kind, share), ts in times.items():
            med = statistics.median(ts)
            print(json.dumps({"skip_empty_env": skip, "empty_wave_first_bounce": bool(live1[((kind, share), "skip")]),
                              "mask": kind, "active_share": share, "ms_per_pass": round(med, 4),
                              "relative_to_full": round(med / base[kind], 4), "spp": a.spp,
                              "second_bounce_paths_per_pass": live1[(kind, share)]}), flush=True)
        pt.free()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
