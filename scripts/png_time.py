"""Device times of the PNG encoder beside today's PNG paths and the JPEG encoder (hipEvents, one process).

    python scripts/png_time.py [--reps 20] [--converged-spp 256] [--grid-only]

Frames: Cornell at 800x800 and 3840x2160, after 1 sample per pixel (mostly black and noisy) and after
--converged-spp samples.  For each frame, the median over --reps warm repetitions of
  stage_ms   the encoder's stages (filter, block, scan, emit, checksums, out) between events on the stream
             (pt_png_enc_profile), and their sum
  total_ms   one pt_preview_png between two events (no profiling events inside)
  wall_ms    PathTracer.preview_png on the host clock: the encode, the copy of the size word and of the file
with the file's size and the share of 8 TB/s that the algorithmic bytes (accumulator read 12 B per pixel, F
written once and read twice, the stream written and read, the file written) make of total_ms.  Beside them,
per frame: today's preview path (pt_preview_rgba, the RGBA8 device-to-host copy, preview.png_bytes on one
core), today's final image (pt_get_image and pt_save_png) against PathTracer.save_png, and pt_preview_jpeg
at quality 90 in 4:2:0.  Then the grid of block_bytes (8 KiB .. 128 KiB) on the 800x800 frames: total_ms and
file size.  --grid-only prints just the grid: with PT_AMD_LIB set to the library that
cuda_pathtracer_amd.build.build_png_chunk_variant(1024) builds, it is the grid's column for the other chunk size C,
a compile-time constant.  One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

import cuda_pathtracer_amd as P  # noqa: E402
from cuda_pathtracer_amd import _native as N  # noqa: E402
from cuda_pathtracer_amd.preview import png_bytes  # noqa: E402

STAGES = ("filter", "block", "scan", "emit", "checksums", "out")
LIB = os.path.basename(os.environ.get("PT_AMD_LIB", "libpt_amd.so"))


def _wall_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


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


def time_png(pt, w, h, spp, reps, torch, block_bytes, stages=True):
    L = P.lib()
    prm = N.PngParams.default()
    prm.block_bytes, prm.mirror_x = block_bytes, 1
    enc = P.PngEncoder(w, h, prm)
    try:
        data = pt.preview_png(spp, enc)
        out, size = enc._buffers()
        st = torch.cuda.current_stream().cuda_stream

        def run():
            N.check_pt(L.pt_preview_png(pt._h, spp, enc._h, out.data_ptr(), enc.cap, size.data_ptr(), st))

        total = _event_ms(run, reps, torch)
        rec = {"what": "png_device", "lib": LIB, "width": w, "height": h, "spp": spp, "block_bytes": block_bytes,
               "reps": reps, "total_ms": round(total, 4), "file_bytes": len(data)}
        if stages:
            N.check_pt(L.pt_png_enc_profile(enc._h, 1))
            per = [[] for _ in STAGES]
            ms = (C.c_float * 6)()
            for _ in range(reps + 3):
                run()
                N.check_pt(L.pt_png_enc_profile_read(enc._h, ms))
                for k in range(6):
                    per[k].append(float(ms[k]))
            N.check_pt(L.pt_png_enc_profile(enc._h, 0))
            wall = _wall_ms(lambda: pt.preview_png(spp, enc), reps)
            stage_ms = {s: round(statistics.median(v[3:]), 4) for s, v in zip(STAGES, per)}
            n_f = h * (1 + 3 * w)
            nbytes = 12 * w * h + 3 * n_f + 2 * (len(data) - 53) + len(data)
            rec.update({"stage_ms": stage_ms, "stage_sum_ms": round(sum(stage_ms.values()), 4),
                        "wall_ms_with_copy": round(wall, 4), "algorithmic_bytes": nbytes,
                        "fraction_of_8TBps": round(nbytes / 8e12 * 1e3 / total, 4)})
        print(json.dumps(rec), flush=True)
        return rec
    finally:
        enc.free()


def time_frame(pt, w, h, spp, reps, torch, tmp):
    L = P.lib()
    rgba = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")

    def png_copy():
        pt.preview_rgba(spp, rgba.data_ptr())
        return rgba.cpu().numpy()

    copy_ms = _wall_ms(png_copy, reps)
    shown = np.ascontiguousarray(png_copy()[:, ::-1, :3])   # the window's orientation, as frame_png encodes it
    png = png_bytes(shown)
    png_ms = _wall_ms(lambda: png_bytes(shown), max(3, reps // 4))
    print(json.dumps({"what": "preview_png_path_today", "width": w, "height": h, "spp": spp, "reps": reps,
                      "rgba_copy_wall_ms": round(copy_ms, 4), "png_bytes_one_core_ms": round(png_ms, 3),
                      "total_ms": round(copy_ms + png_ms, 3), "png_bytes": len(png)}), flush=True)
    rec = time_png(pt, w, h, spp, reps, torch, 32768)
    print(json.dumps({"what": "preview_speedup", "width": w, "height": h, "spp": spp,
                      "today_over_device_wall": round((copy_ms + png_ms) / rec["wall_ms_with_copy"], 1),
                      "device_file_over_todays": round(rec["file_bytes"] / len(png), 4)}), flush=True)
    # the final image: pt_get_image + pt_save_png against PathTracer.save_png (both write the file)
    few = max(3, reps // 4)
    path = str(Path(tmp) / "final.png")
    get_ms = _wall_ms(lambda: pt.image(), few)
    img = pt.image()
    save_ms = _wall_ms(lambda: P.save_image(path, img, float(spp)), few)
    host_size = os.path.getsize(path)
    dev_ms = _wall_ms(lambda: pt.save_png(path, spp), few)
    print(json.dumps({"what": "final_image", "width": w, "height": h, "spp": spp, "reps": few,
                      "get_image_wall_ms": round(get_ms, 3), "save_png_one_core_ms": round(save_ms, 3),
                      "today_ms": round(get_ms + save_ms, 3), "today_file_bytes": host_size,
                      "device_save_png_wall_ms": round(dev_ms, 3), "device_file_bytes": os.path.getsize(path),
                      "today_over_device": round((get_ms + save_ms) / dev_ms, 1)}), flush=True)
    prm = N.JpegParams.default()
    prm.quality, prm.subsampling, prm.mirror_x = 90, N.JPEG_420, 1
    enc = P.JpegEncoder(w, h, prm)
    try:
        data = pt.preview_jpeg(spp, enc)
        out, size = enc._buffers()
        st = torch.cuda.current_stream().cuda_stream
        total = _event_ms(lambda: N.check_pt(L.pt_preview_jpeg(pt._h, spp, enc._h, out.data_ptr(), enc.cap, size.data_ptr(), st)),
                          reps, torch)
        wall = _wall_ms(lambda: pt.preview_jpeg(spp, enc), reps)
        print(json.dumps({"what": "jpeg_q90_420", "width": w, "height": h, "spp": spp, "total_ms": round(total, 4),
                          "wall_ms_with_copy": round(wall, 4), "file_bytes": len(data)}), flush=True)
    finally:
        enc.free()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--converged-spp", type=int, default=256)
    ap.add_argument("--grid-only", action="store_true")
    a = ap.parse_args(argv)
    import torch
    torch.cuda.set_device(0)
    with tempfile.TemporaryDirectory() as tmp:
        for w, h in ((800, 800), (3840, 2160)):
            scene = P.Scene(str(ROOT / "tests" / "scenes" / "cornell.json"))
            scene.set_camera((w, h), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
            scene.finalize()
            pt = P.PathTracer(scene)
            done = 0
            for spp in (1, a.converged_spp):
                for it in range(done + 1, spp + 1):
                    pt.render_pass(it)
                done = spp
                if not a.grid_only:
                    time_frame(pt, w, h, spp, a.reps, torch, tmp)
                for block in (8192, 16384, 32768, 65536, 131072):
                    time_png(pt, w, h, spp, a.reps, torch, block, stages=False)
            pt.free()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
