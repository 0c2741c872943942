"""Device times of the display transform (pt_display): hipEvents around the calls, one process.

    python scripts/display_time.py [--reps 20] [--converged-spp 256] [--meter-only]

Frames: Cornell at 800x800 and 3840x2160, after 1 sample per pixel (mostly black and noisy) and after
--converged-spp samples, and a one-colour image of each size (every lane of the meter hits one bin).  For each
frame, the median over --reps warm repetitions, between two events on the stream, of
  meter_ms        pt_display_meter: the histogram kernel and the one-wave resolve
  resolve_ms      pt_display_meter of a 1 x 1 object: the resolve and the two launches, the histogram kernel idle
  apply_ms        pt_display_apply, RGBA8 out, for the defaults (no curve, linear), ACES + linear and ACES + sRGB
  frame_ms        pt_display_frame (ACES + sRGB, auto)
with the share of 8 TB/s that the bytes they must move make of them: 12 B read per pixel for the meter, 12 B read
and 4 B written for the apply.  Then PathTracer.preview_jpeg without display= (the path of the build before the
display transform) and with it (ACES + sRGB + auto: meter, apply into the encoder's pixels, encode from them), as
event time of the queued work and as wall time with the file's copy.  One JSON line per measurement.

--meter-only: the 1-spp Cornell frame and the one-colour image alone, for a library built with another
PT_DISPLAY_PEEL (build.build_display_variant, selected by PT_AMD_LIB): the measurement behind the number of bins a
wave combines by ballot.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import os  # noqa: E402

import cuda_pathtracer_amd as P  # noqa: E402
from cuda_pathtracer_amd import _native as N  # noqa: E402
from cuda_pathtracer_amd.pathtrace import _jpeg_params  # noqa: E402


def _event_ms(run, reps, torch):
    for _ in range(3):
        run()
    totals = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        totals.append(a.elapsed_time(b))
    return statistics.median(totals)


def _wall_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def _params(**kw):
    p = N.DisplayParams.default()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


LIB = os.path.basename(os.environ.get("PT_AMD_LIB", "libpt_amd.so"))


def _share(nbytes, ms):
    return round(nbytes / 8e12 * 1e3 / ms, 4)


def time_image(what, ptr, w, h, samples, reps, torch, extra=None):
    L = P.lib()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    npix = w * h
    auto = dict(exposure_mode=N.DISPLAY_AUTO)
    objs = {"meter": P.DisplayTransform(w, h, _params(**auto)), "tiny": P.DisplayTransform(1, 1, _params(**auto)),
            "defaults": P.DisplayTransform(w, h, _params()),
            "aces_linear": P.DisplayTransform(w, h, _params(curve=N.DISPLAY_ACES)),
            "aces_srgb": P.DisplayTransform(w, h, _params(curve=N.DISPLAY_ACES, transfer=N.DISPLAY_SRGB)),
            "frame": P.DisplayTransform(w, h, _params(curve=N.DISPLAY_ACES, transfer=N.DISPLAY_SRGB, **auto))}
    try:
        meter = _event_ms(lambda: N.check_pt(L.pt_display_meter(objs["meter"]._h, ptr, samples, st)), reps, torch)
        tiny = _event_ms(lambda: N.check_pt(L.pt_display_meter(objs["tiny"]._h, ptr, samples, st)), reps, torch)
        info = objs["meter"].info()
        row = {"what": what, "lib": LIB, "width": w, "height": h, "samples": samples, "reps": reps, "meter_ms": round(meter, 4),
               "resolve_ms": round(tiny, 4), "meter_fraction_of_8TBps": _share(12 * npix, meter),
               "bins_hit": int(np.count_nonzero(info["hist"])), "largest_bin_share": round(float(info["hist"].max()) / npix, 4),
               "e": info["e"]}
        for name in ("defaults", "aces_linear", "aces_srgb"):
            ms = _event_ms(lambda: N.check_pt(L.pt_display_apply(objs[name]._h, ptr, samples, out.data_ptr(), 4, st)), reps, torch)
            row[f"apply_{name}_ms"] = round(ms, 4)
            row[f"apply_{name}_fraction_of_8TBps"] = _share(16 * npix, ms)
        ms = _event_ms(lambda: N.check_pt(L.pt_display_frame(objs["frame"]._h, ptr, samples, out.data_ptr(), 4, st)), reps, torch)
        row["frame_ms"] = round(ms, 4)
        row.update(extra or {})
        print(json.dumps(row), flush=True)
        return row
    finally:
        for o in objs.values():
            o.free()


def time_preview_jpeg(pt, w, h, spp, reps, torch):
    L = P.lib()
    st = torch.cuda.current_stream().cuda_stream
    enc = P.JpegEncoder(w, h, _jpeg_params(90, "420", True))
    disp = P.DisplayTransform(w, h, _params(exposure_mode=N.DISPLAY_AUTO, rate=32, curve=N.DISPLAY_ACES, transfer=N.DISPLAY_SRGB))
    try:
        out, size = enc._buffers()
        pix = enc._pixel_buffer()

        def plain():
            N.check_pt(L.pt_preview_jpeg(pt._h, spp, enc._h, out.data_ptr(), enc.cap, size.data_ptr(), st))

        def shown():
            N.check_pt(L.pt_preview_display(pt._h, spp, disp._h, pix.data_ptr(), 4, st))
            N.check_pt(L.pt_jpeg_enc_pixels(enc._h, pix.data_ptr(), 4, out.data_ptr(), enc.cap, size.data_ptr(), st))

        a, b = _event_ms(plain, reps, torch), _event_ms(shown, reps, torch)
        wa = _wall_ms(lambda: pt.preview_jpeg(spp, enc), reps)
        na = len(pt.preview_jpeg(spp, enc))
        wb = _wall_ms(lambda: pt.preview_jpeg(spp, enc, display=disp), reps)
        nb = len(pt.preview_jpeg(spp, enc, display=disp))
        print(json.dumps({"what": "preview_jpeg", "width": w, "height": h, "spp": spp, "reps": reps, "quality": 90,
                          "without_display_ms": round(a, 4), "with_display_ms": round(b, 4), "added_ms": round(b - a, 4),
                          "without_display_wall_ms_with_copy": round(wa, 4), "with_display_wall_ms_with_copy": round(wb, 4),
                          "without_display_file_bytes": na, "with_display_file_bytes": nb}), flush=True)
    finally:
        enc.free()
        disp.free()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--converged-spp", type=int, default=256)
    ap.add_argument("--meter-only", action="store_true")
    a = ap.parse_args(argv)
    import torch
    torch.cuda.set_device(0)
    for w, h in ((800, 800), (3840, 2160)):
        scene = P.Scene(str(ROOT / "tests" / "scenes" / "cornell.json"))
        scene.set_camera((w, h), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
        scene.finalize()
        pt = P.PathTracer(scene)
        acc = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        done, cornell = 0, {}
        for spp in (1,) if a.meter_only else (1, a.converged_spp):
            for it in range(done + 1, spp + 1):
                pt.render_pass(it)
            done = spp
            pt.copy_image_to(acc.data_ptr())
            torch.cuda.synchronize()
            cornell[spp] = time_image("cornell", acc.data_ptr(), w, h, float(spp), a.reps, torch)
            if not a.meter_only:
                time_preview_jpeg(pt, w, h, spp, a.reps, torch)
        pt.free()
        acc[:] = torch.tensor([0.3, 0.5, 0.2], device="cuda")
        torch.cuda.synchronize()
        base = cornell[done]["meter_ms"]
        one = time_image("one_colour", acc.data_ptr(), w, h, 1.0, a.reps, torch)
        print(json.dumps({"what": "one_colour_over_cornell", "width": w, "height": h,
                          "meter_ratio": round(one["meter_ms"] / base, 3)}), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
