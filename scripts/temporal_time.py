"""Device times of the temporal reprojection kernels (hipEvents, one process).

    python scripts/temporal_time.py [--reps 20]

pt_temporal_frame in its three cases and pt_temporal_resolve on synthetic planes at 800x800 and
3840x2160, the method of scripts/denoise_time.py: each figure is the median over --reps warm repetitions.
The planes are one surface facing the camera with a band of misses; the new view is the old one turned
by 2.6 pixels and moved a little, so nearly every pixel gathers four taps.  Resolve is timed with every
pixel on the temporal branch of the variance (min_frames = 0) and with every pixel on the spatial one
(min_frames = 2^20).  Algorithmic bytes per pixel (what a kernel must move once; the taps' overlap
between neighbouring lanes is counted once):
  integrate  rgb 12 + prev 12 + H0 16 + H1 8 + mat 4 + alb 16 read, prev 12 + H0 16 + H1 8 written = 104
  reproject  rgb 12 + gA, gB, alb 48 + old H0, H1, gA, gB 56 read, H0, H1, gA, gB, alb, prev 84 written = 200
  empty      rgb 12 + gA, gB, alb 48 read, 84 written = 144
  resolve    H0 16 + H1 8 + mat 4 + alb 16 read, rgb 12 + var 4 + h 4 written = 64
The last column is that traffic at 8 TB/s over the measured time.  Prints one JSON line per measurement.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import cuda_pathtracer_amd as P  # noqa: E402
from cuda_pathtracer_amd import _native as N  # noqa: E402

BYTES = {"integrate": 104, "reproject": 200, "empty": 144, "resolve_temporal": 64, "resolve_spatial": 64}


def _camera(w, h, yaw_pixels=0.0, shift=0.0):
    """A camera at (shift, 0, 5) looking down -z, turned by yaw_pixels pixels about y."""
    c = N.Camera()
    pl = 2 * math.tan(math.radians(25.0)) / h
    a = yaw_pixels * pl
    c.res[:] = [w, h]
    c.position[:] = [shift, 0.0, 5.0]
    c.view[:] = [math.sin(a), 0.0, -math.cos(a)]
    c.right[:] = [math.cos(a), 0.0, math.sin(a)]      # view x (0, 1, 0)
    c.up[:] = [0.0, 1.0, 0.0]
    c.pixel_length[:] = [pl, pl]
    return c


def _planes(cam, w, h, torch, dev):
    """First hits of cam's rays on the plane z = 0 (material 0), a band of misses in world x."""
    x = torch.arange(w, device=dev, dtype=torch.float64)[None, :] - w * 0.5
    y = torch.arange(h, device=dev, dtype=torch.float64)[:, None] - h * 0.5
    view, right, up = (torch.tensor(list(v), device=dev, dtype=torch.float64) for v in (cam.view, cam.right, cam.up))
    d = view - right * cam.pixel_length[0] * x[..., None] - up * cam.pixel_length[1] * y[..., None]
    d = d / d.norm(dim=-1, keepdim=True)
    o = torch.tensor(list(cam.position), device=dev, dtype=torch.float64)
    t = -o[2] / d[..., 2]
    pos = o + d * t[..., None]
    hit = ~((pos[..., 0] > 0.3) & (pos[..., 0] < 0.4))
    gA = torch.zeros((h, w, 4), device=dev)
    gA[..., 2] = hit.float()
    gA[..., 3] = torch.where(hit, 0, -1).to(torch.int32).view(torch.float32)
    gB = torch.zeros((h, w, 4), device=dev)
    gB[..., :3] = (pos * hit[..., None]).float()
    gB[..., 3] = torch.where(hit, t, -1.0).float()
    alb = torch.full((h, w, 4), 0.7, device=dev)
    return gA, gB, alb, float(hit.float().mean())


def _median_ms(fn, prepare, reps, torch):
    ts = []
    for i in range(reps + 3):
        prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= 3:   # (the first three warm up)
            ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def time_size(w, h, reps, torch):
    L = P.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    rgb1 = torch.rand((h, w, 3), device=dev, generator=g) * 2
    rgb2 = rgb1 + torch.rand((h, w, 3), device=dev, generator=g) * 2
    cam_a, cam_b = _camera(w, h), _camera(w, h, yaw_pixels=2.6, shift=0.02)
    pa, pb = _planes(cam_a, w, h, torch, dev), _planes(cam_b, w, h, torch, dev)
    st = torch.cuda.current_stream().cuda_stream
    prm = N.TemporalParams.default()
    t = C.c_void_p()
    N.check_pt(L.pt_temporal_create(w, h, C.byref(prm), C.byref(t)))
    out_rgb = torch.empty((h, w, 3), device=dev)
    out_var, out_h = torch.empty((h, w), device=dev), torch.empty((h, w), device=dev)

    def frame(cam, rgb, samples, pl):
        N.check_pt(L.pt_temporal_frame(t, C.byref(cam), rgb.data_ptr(), samples, pl[0].data_ptr(), pl[1].data_ptr(),
                                       pl[2].data_ptr(), st))

    def at_a():   # a history of one frame at A
        N.check_pt(L.pt_temporal_reset(t))
        frame(cam_a, rgb1, 1.0, pa)

    def case():
        k = C.c_int32()
        N.check_pt(L.pt_temporal_info(t, None, None, C.byref(k)))
        return k.value

    rows = {}
    try:
        rows["empty"] = _median_ms(lambda: frame(cam_a, rgb1, 1.0, pa), lambda: N.check_pt(L.pt_temporal_reset(t)), reps, torch)
        assert case() == 1
        rows["integrate"] = _median_ms(lambda: frame(cam_a, rgb2, 2.0, pa), at_a, reps, torch)
        assert case() == 2
        rows["reproject"] = _median_ms(lambda: frame(cam_b, rgb1, 1.0, pb), at_a, reps, torch)
        assert case() == 3
        N.check_pt(L.pt_temporal_resolve(t, out_rgb.data_ptr(), out_var.data_ptr(), out_h.data_ptr(), st))
        kept = float((out_h > 1).float().mean())
        for name, mf in (("resolve_temporal", 0), ("resolve_spatial", 1 << 20)):
            N.check_pt(L.pt_temporal_destroy(t))
            prm.min_frames = mf
            N.check_pt(L.pt_temporal_create(w, h, C.byref(prm), C.byref(t)))
            at_a()
            rows[name] = _median_ms(lambda: N.check_pt(L.pt_temporal_resolve(t, out_rgb.data_ptr(), out_var.data_ptr(),
                                                                             out_h.data_ptr(), st)), lambda: None, reps, torch)
    finally:
        N.check_pt(L.pt_temporal_destroy(t))
    for name, ms in rows.items():
        nbytes = BYTES[name] * w * h
        print(json.dumps({"what": "temporal_" + name, "width": w, "height": h, "reps": reps, "ms": round(ms, 4),
                          "bytes_per_pixel": BYTES[name], "fraction_of_8TBps": round(nbytes / 8e12 * 1e3 / ms, 3),
                          "hit_fraction": round(pb[3], 4), "kept_fraction_after_move": round(kept, 4)}), flush=True)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args(argv)
    import torch
    torch.cuda.set_device(0)
    for w, h in ((800, 800), (3840, 2160)):
        time_size(w, h, a.reps, torch)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
