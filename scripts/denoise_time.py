"""Device times of the a-trous denoiser and the G-buffer kernel (hipEvents, one process).

    python scripts/denoise_time.py [--reps 20]

Denoiser: pt_denoiser_run on synthetic planes at 800x800 and 3840x2160, for levels = 0..5; the time of
level i is t(i + 1 levels) - t(i levels) (the last launch of a run is the variant that fuses the
remodulation and the float3 store).  Each figure is the median over --reps warm repetitions.  The
algorithmic traffic of a level is 64 B per pixel (three 16-byte reads, one 16-byte write); the last
column is that traffic at 8 TB/s over the measured time.
The variance-guided filter (pt_denoiser_run_var) is timed beside the plain one in the same loop (plain and
variance-guided runs alternate per level count); each level's ratio to the plain level of the same run
is printed.
Moments: pt_moments_update at both sizes, with and without albedo (its traffic: rgb 12 + prev/m1 16 + m2 4
[+ alb 16] read, 20 written, per pixel), as a fraction of 8 TB/s.
Tracking: the drop-in call sequence (flags, pass, render-ahead, image copy) on Cornell 800x800 with and
without one pt_variance_update per pass, alternating blocks in one process, wall clock per iteration.
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
    var = torch.rand((h, w), device=dev, generator=g) * 0.05
    out_var = torch.empty((h, w), device=dev)
    dn = C.c_void_p()
    N.check_pt(L.pt_denoiser_create(w, h, C.byref(dn)))
    st = torch.cuda.current_stream().cuda_stream
    total, total_var = [], []
    try:
        for levels in range(6):
            prm = N.DenoiseParams.default()
            prm.levels = levels
            vprm = N.DenoiseVarParams.default()
            vprm.levels = levels

            def run():
                N.check_pt(L.pt_denoiser_run(dn, rgb.data_ptr(), 16.0, gA.data_ptr(), gB.data_ptr(), alb.data_ptr(),
                                             C.byref(prm), out.data_ptr(), st))

            def run_var():
                N.check_pt(L.pt_denoiser_run_var(dn, rgb.data_ptr(), 16.0, var.data_ptr(), gA.data_ptr(), gB.data_ptr(),
                                                 alb.data_ptr(), C.byref(vprm), out.data_ptr(), out_var.data_ptr(), st))

            total.append(_median_ms(run, reps, torch))
            total_var.append(_median_ms(run_var, reps, torch))
    finally:
        L.pt_denoiser_destroy(dn)
    per_level = [total[i + 1] - total[i] for i in range(5)]
    ideal_ms = 64.0 * w * h / 8e12 * 1e3
    lv = [total_var[i + 1] - total_var[i] for i in range(5)]
    print(json.dumps({"what": "denoiser_var", "width": w, "height": h, "reps": reps,
                      "total_ms_by_levels": [round(t, 4) for t in total_var],
                      "level_ms": [round(t, 4) for t in lv],
                      "level_ratio_to_plain": [round(a / b, 3) if b > 0 else None for a, b in zip(lv, per_level)],
                      "total5_ratio_to_plain": round(total_var[5] / total[5], 3)}), flush=True)
    print(json.dumps({"what": "denoiser", "width": w, "height": h, "reps": reps,
                      "total_ms_by_levels": [round(t, 4) for t in total],
                      "level_ms": [round(t, 4) for t in per_level],
                      "ideal_level_ms_at_8TBps": round(ideal_ms, 5),
                      "fraction_of_8TBps": [round(ideal_ms / t, 3) if t > 0 else None for t in per_level],
                      "total5_fraction_of_8TBps": round(5 * ideal_ms / total[5], 3)}), flush=True)


def time_moments(w, h, reps, torch):
    L = P.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    rgb = torch.rand((h, w, 3), device=dev, generator=g) * 4
    alb = torch.full((h, w, 4), 0.7, device=dev)
    m = C.c_void_p()
    N.check_pt(L.pt_moments_create(w, h, C.byref(m)))
    st = torch.cuda.current_stream().cuda_stream
    try:
        for with_alb in (False, True):
            N.check_pt(L.pt_moments_reset(m, None, st))
            ms = _median_ms(lambda: N.check_pt(L.pt_moments_update(m, rgb.data_ptr(), 1.0,
                                                                   alb.data_ptr() if with_alb else None, st)), reps, torch)
            nbytes = (12 + 16 + 4 + (16 if with_alb else 0) + 20) * w * h
            print(json.dumps({"what": "moments_update", "width": w, "height": h, "albedo": with_alb, "reps": reps,
                              "ms": round(ms, 4), "bytes_per_pixel": nbytes // (w * h),
                              "fraction_of_8TBps": round(nbytes / 8e12 * 1e3 / ms, 3)}), flush=True)
    finally:
        L.pt_moments_destroy(m)


def time_tracking(path, blocks, iters_per_block, torch):
    """The drop-in sequence per iteration, untracked and tracked contexts in alternating blocks."""
    import time
    scene = P.Scene(path)
    gui = P.GuiDataContainer()
    ctx = {False: P.PathTracer(scene, gui), True: P.PathTracer(scene, gui)}
    ctx[True].track_variance(True)
    it = {False: 0, True: 0}
    per_iter = {False: [], True: []}
    for b in range(2 * blocks + 2):
        tracked = bool(b & 1)
        pt = ctx[tracked]
        t0 = time.perf_counter()
        for _ in range(iters_per_block):
            it[tracked] += 1
            pt.set_flags(gui)
            pt.render_pass(it[tracked])
            if tracked:
                pt.variance_update()
            pt.render_ahead(it[tracked] + 1)
            pt.image()
        if b >= 2:   # (the first block of each is the warm-up)
            per_iter[tracked].append((time.perf_counter() - t0) / iters_per_block * 1e3)
    same = ctx[False].image().tobytes() == ctx[True].image().tobytes()
    for pt in ctx.values():
        pt.free()
    a, t = statistics.median(per_iter[False]), statistics.median(per_iter[True])
    print(json.dumps({"what": "tracking_in_dropin_loop", "width": 800, "height": 800, "blocks": blocks,
                      "iters_per_block": iters_per_block, "untracked_ms_per_iter": round(a, 4),
                      "tracked_ms_per_iter": round(t, 4), "ratio": round(t / a, 3),
                      "untracked_blocks_ms": [round(v, 4) for v in per_iter[False]],
                      "tracked_blocks_ms": [round(v, 4) for v in per_iter[True]], "same_image": same}), flush=True)


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
        time_moments(w, h, a.reps, torch)
    time_tracking(str(ROOT / "tests" / "scenes" / "cornell.json"), 5, 100, torch)
    time_gbuffer("cornell_800x800", str(ROOT / "tests" / "scenes" / "cornell.json"), a.reps, torch)
    with tempfile.TemporaryDirectory() as tmp:
        time_gbuffer("random_triangles_100k", scenes.random_triangles(tmp), a.reps, torch)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
