"""Device times of the a-trous denoiser and the G-buffer kernel (hipEvents, one process).

    python scripts/denoise_time.py [--reps 20]

Denoiser: pt_denoiser_run on synthetic planes at 800x800 and 3840x2160, for levels = 0..5; the time of
level i is t(i + 1 levels) - t(i levels) (the last launch of a run is the variant that fuses the
remodulation and the float3 store).  Each figure is the median over --reps warm repetitions.  The
algorithmic traffic of a level is 64 B per pixel (three 16-byte reads, one 16-byte write); the last
column is that traffic at 8 TB/s over the measured time.
G-buffer: pt_gbuffer on Cornell 800x800 and on the 100k-triangle scene (scenes.random_triangles).
Prints one JSON line per measurement.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import cuda_pathtracer_amd as P  # noqa: E402
from cuda_pathtracer_amd import _native as N  # noqa: E402
from cuda_pathtracer_amd import scenes  # noqa: E402


def _median_ms(fn, reps, torch):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def time_denoiser(w, h, reps, torch):
    L = P.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    rgb = torch.rand((h, w, 3), device=dev, generator=g) * 4
    gA = torch.zeros((h, w, 4), device=dev)
    gA[..., 2] = 1.0                              # one plane facing the camera, material id 0
    gB = torch.zeros((h, w, 4), device=dev)
    gB[..., 0] = torch.arange(w, device=dev)[None, :] * 0.01
    gB[..., 1] = torch.arange(h, device=dev)[:, None] * 0.01
    gB[..., 3] = 5.0
    alb = torch.full((h, w, 4), 0.7, device=dev)
    out = torch.empty((h, w, 3), device=dev)
    dn = C.c_void_p()
    N.check_pt(L.pt_denoiser_create(w, h, C.byref(dn)))
    st = torch.cuda.current_stream().cuda_stream
    total = []
    try:
        for levels in range(6):
            prm = N.DenoiseParams.default()
            prm.levels = levels

            def run():
                N.check_pt(L.pt_denoiser_run(dn, rgb.data_ptr(), 16.0, gA.data_ptr(), gB.data_ptr(), alb.data_ptr(),
                                             C.byref(prm), out.data_ptr(), st))

            total.append(_median_ms(run, reps, torch))
    finally:
        L.pt_denoiser_destroy(dn)
    per_level = [total[i + 1] - total[i] for i in range(5)]
    ideal_ms = 64.0 * w * h / 8e12 * 1e3
    print(json.dumps({"what": "denoiser", "width": w, "height": h, "reps": reps,
                      "total_ms_by_levels": [round(t, 4) for t in total],
                      "level_ms": [round(t, 4) for t in per_level],
                      "ideal_level_ms_at_8TBps": round(ideal_ms, 5),
                      "fraction_of_8TBps": [round(ideal_ms / t, 3) if t > 0 else None for t in per_level],
                      "total5_fraction_of_8TBps": round(5 * ideal_ms / total[5], 3)}), flush=True)


def time_gbuffer(name, path, reps, torch):
    scene = P.Scene(path)
    pt = P.PathTracer(scene)
    dev = torch.device("cuda", 0)
    planes = [torch.empty((pt.npix, 4), device=dev) for _ in range(3)]
    uv = torch.empty((pt.npix, 2), device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def run():
        N.check_pt(P.lib().pt_gbuffer(pt._h, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(),
                                      uv.data_ptr(), st))

    ms = _median_ms(run, reps, torch)
    hit = float((planes[1][:, 3] > 0).float().mean())
    print(json.dumps({"what": "gbuffer", "scene": name, "width": pt.width, "rows": pt.rows, "reps": reps,
                      "ms": round(ms, 4), "hit_fraction": round(hit, 4)}), flush=True)
    pt.free()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args(argv)
    import torch
    torch.cuda.set_device(0)
    for w, h in ((800, 800), (3840, 2160)):
        time_denoiser(w, h, a.reps, torch)
    time_gbuffer("cornell_800x800", str(ROOT / "tests" / "scenes" / "cornell.json"), a.reps, torch)
    with tempfile.TemporaryDirectory() as tmp:
        time_gbuffer("random_triangles_100k", scenes.random_triangles(tmp), a.reps, torch)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
