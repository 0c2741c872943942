"""Device times of the JPEG encoder beside today's PNG frame path (hipEvents, one process).

    python scripts/jpeg_time.py [--reps 20] [--converged-spp 256]

Frames: Cornell at 800x800 and 3840x2160, after 1 sample per pixel (noisy: the entropy coder's worst
frame of a render) and after --converged-spp samples.  For each frame, quality 50 and 90 in 4:4:4 and
4:2:0: the median over --reps warm repetitions of
  stage_ms   the encoder's stages (blocks, count, scan, emit, stuff) between events on the stream
             (pt_jpeg_enc_profile), and their sum
  total_ms   one pt_preview_jpeg between two events (no profiling events inside)
  wall_ms    PathTracer.preview_jpeg on the host clock: the encode, the copy of the size word and of
             the file's bytes
with the file's size and the share of 8 TB/s that the algorithmic bytes (accumulator read 12 B per
pixel, coefficients written once and read twice, unstuffed stream written and read, file written) make
of total_ms.  Beside them, per frame, today's path: pt_preview_rgba and the RGBA8 device-to-host copy
(wall clock) and preview.png_bytes of the frame on one core.  Prints one JSON line per measurement.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

import cuda_pathtracer_amd as P  # noqa: E402
from cuda_pathtracer_amd import _native as N  # noqa: E402
from cuda_pathtracer_amd.preview import png_bytes  # noqa: E402

STAGES = ("blocks", "count", "scan", "emit", "stuff")


def _wall_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def time_frame(pt, w, h, spp, reps, torch):
    L = P.lib()
    rgba = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")

    def png_copy():
        pt.preview_rgba(spp, rgba.data_ptr())
        return rgba.cpu().numpy()

    copy_ms = _wall_ms(png_copy, reps)
    shown = np.ascontiguousarray(png_copy()[:, ::-1, :3])   # the window's orientation, as frame_png encodes it
    png = png_bytes(shown)
    png_ms = _wall_ms(lambda: png_bytes(shown), max(3, reps // 4))
    print(json.dumps({"what": "png_path", "width": w, "height": h, "spp": spp, "reps": reps,
                      "rgba_copy_wall_ms": round(copy_ms, 4), "png_bytes_one_core_ms": round(png_ms, 3),
                      "total_ms": round(copy_ms + png_ms, 3), "rgba_bytes": w * h * 4, "png_bytes": len(png)}), flush=True)
    for quality in (50, 90):
        for sub, name in ((N.JPEG_444, "444"), (N.JPEG_420, "420")):
            prm = N.JpegParams.default()
            prm.quality, prm.subsampling, prm.mirror_x = quality, sub, 1
            enc = P.JpegEncoder(w, h, prm)
            try:
                data = pt.preview_jpeg(spp, enc)
                out, size = enc._buffers()
                st = torch.cuda.current_stream().cuda_stream

                def run():
                    N.check_pt(L.pt_preview_jpeg(pt._h, spp, enc._h, out.data_ptr(), enc.cap, size.data_ptr(), st))

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
                N.check_pt(L.pt_jpeg_enc_profile(enc._h, 1))
                stages = [[] for _ in STAGES]
                ms = (C.c_float * 5)()
                for _ in range(reps + 3):
                    run()
                    N.check_pt(L.pt_jpeg_enc_profile_read(enc._h, ms))
                    for k in range(5):
                        stages[k].append(float(ms[k]))
                N.check_pt(L.pt_jpeg_enc_profile(enc._h, 0))
                wall = _wall_ms(lambda: pt.preview_jpeg(spp, enc), reps)
                stage_ms = {s: round(statistics.median(v[3:]), 4) for s, v in zip(STAGES, stages)}
                m = 8 if sub == N.JPEG_444 else 16
                blocks = (3 if m == 8 else 6) * ((w + m - 1) // m) * ((h + m - 1) // m)
                unstuffed = len(data[623:-2].replace(b"\xff\x00", b"\xff"))
                nbytes = 12 * w * h + 3 * 128 * blocks + 2 * unstuffed + len(data)
                total = statistics.median(totals)
                print(json.dumps({"what": "jpeg", "width": w, "height": h, "spp": spp, "quality": quality,
                                  "subsampling": name, "reps": reps, "stage_ms": stage_ms,
                                  "stage_sum_ms": round(sum(stage_ms.values()), 4), "total_ms": round(total, 4),
                                  "wall_ms_with_copy": round(wall, 4), "file_bytes": len(data),
                                  "algorithmic_bytes": nbytes,
                                  "fraction_of_8TBps": round(nbytes / 8e12 * 1e3 / total, 4),
                                  "png_path_over_jpeg_wall": round((copy_ms + png_ms) / wall, 1)}), flush=True)
            finally:
                enc.free()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--converged-spp", type=int, default=256)
    a = ap.parse_args(argv)
    import torch
    torch.cuda.set_device(0)
    for w, h in ((800, 800), (3840, 2160)):
        scene = P.Scene(str(ROOT / "tests" / "scenes" / "cornell.json"))
        scene.set_camera((w, h), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
        scene.finalize()
        pt = P.PathTracer(scene)
        pt.render_pass(1)
        time_frame(pt, w, h, 1, a.reps, torch)
        for it in range(2, a.converged_spp + 1):
            pt.render_pass(it)
        time_frame(pt, w, h, a.converged_spp, a.reps, torch)
        pt.free()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
