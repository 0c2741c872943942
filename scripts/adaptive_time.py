"""Device times of the adaptive-sampling kernels (hipEvents, one process).

    python scripts/adaptive_time.py [--reps 20]

pt_adaptive's update, select and resolve on synthetic accumulators at 800x800 and 3840x2160, the method
of scripts/denoise_time.py: each figure is the median over --reps warm repetitions.  update is timed
with every block active and with a random half of them (with the albedo division); select (k_ad_hot +
k_ad_dilate) at dilate 1 on the moments those updates left.  Algorithmic bytes per pixel (what a kernel
must move once; the per-block words are 1/64 of a pixel's and not counted, the dilation box's overlap
between neighbouring lanes is counted once):
  update   rgb 12 + alb 16 + (prev, m1) 16 + m2 4 read, (prev, m1) 16 + m2 4 written = 68 per active pixel
  select   (prev, m1) 16 + m2 4 read, hot 1 written; hot 1 read = 22
  resolve  rgb 12 + (prev, m1) 16 + m2 4 read, rgb 12 + var 4 written = 48
The last column is that traffic at 8 TB/s over the measured time.  Prints one JSON line per measurement.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import cuda_pathtracer_amd as P  # noqa: E402
from cuda_pathtracer_amd import _native as N  # noqa: E402

BYTES = {"update_all": 68, "update_half": 34, "select": 22, "resolve": 48}


def _median_ms(fn, reps, torch):
    ts = []
    for i in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= 3:   # (the first three warm up)
            ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def time_size(w, h, reps, torch):
    import numpy as np
    L = P.lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(5)
    rgb = [torch.rand((h, w, 3), device=dev, generator=g) * (k + 1) for k in range(2)]
    alb = torch.rand((h, w, 4), device=dev, generator=g) * 0.9 + 0.05
    out_rgb, out_var = torch.empty((h, w, 3), device=dev), torch.empty((h, w), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    a = C.c_void_p()
    N.check_pt(L.pt_adaptive_obj_create(w, h, C.byref(a)))
    nblk = (w * h + 63) // 64
    prm = N.AdaptiveParams.default()
    prm.dilate = 1
    k = [0]

    def update():
        k[0] ^= 1
        N.check_pt(L.pt_adaptive_obj_update(a, rgb[k[0]].data_ptr(), 4.0, alb.data_ptr(), st))

    rows = {}
    try:
        N.check_pt(L.pt_adaptive_obj_reset(a, None, st))
        rows["update_all"] = _median_ms(update, reps, torch)
        half = (np.random.default_rng(1).random(nblk) < 0.5).astype(np.uint8)
        N.check_pt(L.pt_adaptive_obj_set_mask(a, half.ctypes.data, nblk, st))
        rows["update_half"] = _median_ms(update, reps, torch)
        active = C.c_int32()
        rows["select"] = _median_ms(lambda: N.check_pt(L.pt_adaptive_obj_select(a, C.byref(prm), st, None, None)), reps, torch)
        N.check_pt(L.pt_adaptive_obj_select(a, C.byref(prm), st, C.byref(active), None))
        rows["resolve"] = _median_ms(lambda: N.check_pt(L.pt_adaptive_obj_resolve(a, rgb[0].data_ptr(), out_rgb.data_ptr(),
                                                                                 out_var.data_ptr(), st)), reps, torch)
    finally:
        N.check_pt(L.pt_adaptive_obj_destroy(a))
    for name, ms in rows.items():
        nbytes = BYTES[name] * w * h
        print(json.dumps({"what": "adaptive_" + name, "width": w, "height": h, "reps": reps, "ms": round(ms, 4),
                          "bytes_per_pixel": BYTES[name], "fraction_of_8TBps": round(nbytes / 8e12 * 1e3 / ms, 3),
                          "active_blocks_after_select": active.value, "blocks": nblk}), flush=True)


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
