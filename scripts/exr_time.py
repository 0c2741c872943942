"""Device times of the OpenEXR encoder (hipEvents, one process).

    python scripts/exr_time.py [--reps 20] [--converged-spp 64]

Frames: Cornell at 800x800 and 3840x2160, after 1 sample per pixel (noisy: many chunks fall back to raw bytes) and after
--converged-spp samples.  For each frame and each of the files
  beauty_float_zip, beauty_half_zip, beauty_float_zips, beauty_float_none, all_float_zip (the 16 channels of every layer)
the median over --reps warm repetitions of
  stage_ms   the encoder's stages (convert, block, scan, emit, checksums, out) between events on the stream
             (pt_exr_enc_profile), and their sum
  total_ms   one pt_preview_exr between two events (no profiling events inside; with the other layers it includes
             pt_gbuffer)
  wall_ms    PathTracer.preview_exr on the host clock: the encode, the copy of the size word and of the file
with the file's size, its bound, the number of raw chunks, and beside them the copy of the accumulator to the host
(pt_get_image), which any host writer would need first.  The file is read back by tests/exr_ref.py's reader and its beauty
compared with the accumulator.  One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import ctypes as C
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
from cuda_pathtracer_amd import _native as N  # noqa: E402
from tests import exr_ref as R  # noqa: E402

STAGES = ("convert", "block", "scan", "emit", "checksums", "out")
LIB = os.path.basename(os.environ.get("PT_AMD_LIB", "libpt_amd.so"))
FILES = {"beauty_float_zip": (P.EXR_BEAUTY, 0, N.EXR_ZIP), "beauty_half_zip": (P.EXR_BEAUTY, P.EXR_BEAUTY, N.EXR_ZIP),
         "beauty_float_zips": (P.EXR_BEAUTY, 0, N.EXR_ZIPS), "beauty_float_none": (P.EXR_BEAUTY, 0, N.EXR_NONE),
         "all_float_zip": (P.EXR_ALL_LAYERS, 0, N.EXR_ZIP)}


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


def time_file(pt, w, h, spp, name, reps, torch, accum) -> bool:
    L = P.lib()
    layers, half, comp = FILES[name]
    prm = N.ExrParams.default()
    prm.compression, prm.mirror_x = comp, 1
    enc = P.ExrEncoder(w, h, P.exr_ctx_channels(layers, half), prm)
    try:
        data = pt.preview_exr(spp, enc, layers)
        out, size = enc._buffers()
        st = torch.cuda.current_stream().cuda_stream

        def run():
            N.check_pt(L.pt_preview_exr(pt._h, spp, layers, enc._h, out.data_ptr(), enc.cap, size.data_ptr(), st))

        total = _event_ms(run, reps, torch)
        N.check_pt(L.pt_exr_enc_profile(enc._h, 1))
        per = [[] for _ in STAGES]
        ms = (C.c_float * 6)()
        for _ in range(reps + 3):
            run()
            N.check_pt(L.pt_exr_enc_profile_read(enc._h, ms))
            for k in range(6):
                per[k].append(float(ms[k]))
        N.check_pt(L.pt_exr_enc_profile(enc._h, 0))
        wall = _wall_ms(lambda: pt.preview_exr(spp, enc, layers), reps)
    finally:
        enc.free()
    info = {}
    dec = R.read_exr(data, info)
    want = (accum / np.float32(spp))[:, ::-1]
    same = all((dec[c].view(np.uint16) == R.half_bits(np.ascontiguousarray(want[..., k]).view(np.uint32))).all() if half
               else (dec[c] == want[..., k]).all() for k, c in enumerate("RGB"))
    stage_ms = {s: round(statistics.median(v[3:]), 4) for s, v in zip(STAGES, per)}
    print(json.dumps({"what": "exr_device", "file": name, "lib": LIB, "width": w, "height": h, "spp": spp, "reps": reps,
                      "total_ms": round(total, 4), "stage_ms": stage_ms, "stage_sum_ms": round(sum(stage_ms.values()), 4),
                      "binding_stage": max(stage_ms, key=stage_ms.get), "wall_ms_with_copy": round(wall, 4),
                      "file_bytes": len(data), "bound_bytes": enc.bound, "chunks": len(info["raw"]),
                      "raw_chunks": int(sum(info["raw"])), "beauty_read_back_equal": bool(same)}), flush=True)
    return bool(same)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--converged-spp", type=int, default=64)
    a = ap.parse_args(argv)
    import torch
    torch.cuda.set_device(0)
    ok = True
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
            accum = pt.image()
            get_ms = _wall_ms(lambda: pt.image(), a.reps)
            print(json.dumps({"what": "accumulator_to_host", "width": w, "height": h, "spp": spp,
                              "get_image_wall_ms": round(get_ms, 3), "accum_bytes": 12 * w * h}), flush=True)
            for name in FILES:
                ok = time_file(pt, w, h, spp, name, a.reps, torch, accum) and ok
        pt.free()
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
