"""Device times of the Radiance HDR encoder beside today's host path (hipEvents, one process).

    python scripts/hdr_time.py [--reps 20] [--converged-spp 256]

Frames: Cornell at 800x800 and 3840x2160, after 1 sample per pixel (mostly black and noisy) and after
--converged-spp samples.  For each frame, the median over --reps warm repetitions of
  stage_ms   the encoder's stages (convert, count, scan, emit) between events on the stream
             (pt_hdr_enc_profile), and their sum
  total_ms   one pt_preview_hdr between two events (no profiling events inside)
  wall_ms    PathTracer.preview_hdr on the host clock: the encode, the copy of the size word and of the file
with the file's size and the share of 8 TB/s that the algorithmic bytes (accumulator read 12 B per pixel, the
planes written once and read twice 4 B per pixel each time, the file written) make of total_ms.  Beside them, in
the same call, today's path, which this work leaves unchanged: pt_get_accum (the accumulator's copy to the host)
and pt_encode_hdr on one core; the two files are compared.  One JSON line per measurement.
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

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import cuda_pathtracer_amd as P  # noqa: E402
from cuda_pathtracer_amd import _native as N  # noqa: E402

STAGES = ("convert", "count", "scan", "emit")
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


def time_frame(pt, w, h, spp, reps, torch):
    L = P.lib()
    prm = N.HdrParams.default()
    prm.mirror_x = 1
    enc = P.HdrEncoder(w, h, prm)
    try:
        data = pt.preview_hdr(spp, enc)
        out, size = enc._buffers()
        st = torch.cuda.current_stream().cuda_stream

        def run():
            N.check_pt(L.pt_preview_hdr(pt._h, spp, enc._h, out.data_ptr(), enc.cap, size.data_ptr(), st))

        total = _event_ms(run, reps, torch)
        N.check_pt(L.pt_hdr_enc_profile(enc._h, 1))
        per = [[] for _ in STAGES]
        ms = (C.c_float * 4)()
        for _ in range(reps + 3):
            run()
            N.check_pt(L.pt_hdr_enc_profile_read(enc._h, ms))
            for k in range(4):
                per[k].append(float(ms[k]))
        N.check_pt(L.pt_hdr_enc_profile(enc._h, 0))
        wall = _wall_ms(lambda: pt.preview_hdr(spp, enc), reps)
        stage_ms = {s: round(statistics.median(v[3:]), 4) for s, v in zip(STAGES, per)}
        nbytes = 12 * w * h + 3 * 4 * w * h + len(data)
        print(json.dumps({"what": "hdr_device", "lib": LIB, "width": w, "height": h, "spp": spp, "reps": reps,
                          "total_ms": round(total, 4), "stage_ms": stage_ms, "stage_sum_ms": round(sum(stage_ms.values()), 4),
                          "binding_stage": max(stage_ms, key=stage_ms.get), "wall_ms_with_copy": round(wall, 4),
                          "file_bytes": len(data), "bound_bytes": enc.bound, "algorithmic_bytes": nbytes,
                          "fraction_of_8TBps": round(nbytes / 8e12 * 1e3 / total, 4)}), flush=True)
    finally:
        enc.free()
    # today's path: the accumulator to the host, then the scalar writer
    few = max(3, reps // 4)
    get_ms = _wall_ms(lambda: pt.image(), reps)
    img = pt.image()
    enc_ms = _wall_ms(lambda: P.encode_hdr(img, float(spp)), few)
    same = P.encode_hdr(img, float(spp)) == data
    print(json.dumps({"what": "hdr_host_path_today", "width": w, "height": h, "spp": spp, "reps": reps, "encode_reps": few,
                      "get_accum_wall_ms": round(get_ms, 3), "accum_bytes": 12 * w * h, "encode_hdr_one_core_ms": round(enc_ms, 3),
                      "today_ms": round(get_ms + enc_ms, 3), "files_equal": same,
                      "device_total_below_accum_copy": total < get_ms,
                      "today_over_device_wall": round((get_ms + enc_ms) / wall, 1)}), flush=True)
    return same


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--converged-spp", type=int, default=256)
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
            ok = time_frame(pt, w, h, spp, a.reps, torch) and ok
        pt.free()
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
