"""Device times of the bloom (pt_bloom): hipEvents around pt_bloom_apply, one process.

    python scripts/bloom_time.py [--reps 20] [--levels 6]

Images of 800x800 and 3840x2160 (2^uniform(-6, 6) per channel: about a third of the pixels glare at the default
threshold).  For each, the median over --reps warm repetitions, between two events on the stream, of one
pt_bloom_apply out of place, and of the parts a pyramid of fewer levels isolates (levels = 1: k_bloom_first and
k_bloom_compose alone), with the share of 8 TB/s that the bytes the definition must move make of the time: 12 B read
and 12 B written per pixel, and per 16-byte texel of the levels n_1 .. n_K
  written   n_1 .. n_K by the down steps, n_1 .. n_K-1 again by the up steps
  read      n_1 .. n_K-1 by the down steps, n_k+1 and n_k by the up step k, n_1 by the composition.
One JSON line per measurement, with the loaded library's name (PT_AMD_LIB selects another build).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import cuda_pathtracer_amd as P  # noqa: E402
from cuda_pathtracer_amd import _native as N  # noqa: E402

LIB = os.path.basename(os.environ.get("PT_AMD_LIB", "libpt_amd.so"))


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
    return statistics.median(totals), min(totals), max(totals)


def bytes_moved(w: int, h: int, info: dict) -> int:
    n = [wk * hk for wk, hk in zip(info["widths"], info["heights"])]
    k = len(n)
    written = sum(n) + sum(n[:k - 1])
    read = sum(n[:k - 1]) + sum(n[j + 1] + n[j] for j in range(k - 1)) + n[0]
    return 24 * w * h + 16 * (written + read)


def time_size(w, h, levels, reps, torch):
    L = P.lib()
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(w)
    src = torch.exp2(torch.rand((h, w, 3), device="cuda", generator=gen) * 12.0 - 6.0)
    out = torch.empty_like(src)
    for lv in sorted({1, 2, levels}):
        prm = N.BloomParams.default()
        prm.levels = lv
        b = P.Bloom(w, h, prm)
        try:
            med, lo, hi = _event_ms(lambda: N.check_pt(L.pt_bloom_apply(b._h, src.data_ptr(), 1.0, out.data_ptr(), st)), reps, torch)
            nbytes = bytes_moved(w, h, b.info())
            print(json.dumps({"what": "bloom_apply", "lib": LIB, "width": w, "height": h, "levels": lv, "reps": reps,
                              "ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), "launches": 2 * lv,
                              "bytes": nbytes, "fraction_of_8TBps": round(nbytes / 8e12 * 1e3 / med, 4)}), flush=True)
        finally:
            b.free()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--levels", type=int, default=6)
    a = ap.parse_args(argv)
    import torch
    torch.cuda.set_device(0)
    for w, h in ((800, 800), (3840, 2160)):
        time_size(w, h, a.levels, a.reps, torch)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
