#!/usr/bin/env python3
"""Device-resident throughput of the quality metric (icamd_measure_error_device, include/ic_amd.h).

Legs, each at 16 x 4096^2: DXT1 <- RGBA8, DXT5, ETC1 <- RGB888, PVRTC 2 bpp.  Three variants per leg, timed in the same run:
  (a) metric   icamd_measure_error_device on the encoder's blocks and the source pixels
  (b) detour   what a caller had to do without it: icamd_decode_device into a pixel buffer, then a torch reduction of the
               squared difference against the source (per-image sums over every decoded channel)
  (c) encode   icamd_encode_device of the same launch shape (ETC1: kHeuristic)
(b) and (c) are the yardsticks.  Method (scripts/bench_bc45.py): about a second of untimed launches of the variant
first (the chip ramps its power state out of idle), then device events around K back-to-back calls, repeated; the median and
min / max of ms per call.  Algorithmic bytes of (a) = source and blocks read once, nothing written, against 8 TB/s.
Parity per leg: (a)'s sums of squares against (b)'s for every image, and image 0 against the definition computed with the
oracle's decoder (tests/metric_oracle.py: test infrastructure, the checker only).

  python scripts/bench_metric.py [--k 20] [--reps 7] [--size 4096] [--n 16] [--legs dxt1,dxt5,etc1,pvrtc2] [--out FILE]
One JSON line per leg (also appended to --out); exit status 1 if any parity check fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ic_amd_loader  # noqa: E402

pkg = ic_amd_loader.load_package()
import ic_testlib as T  # noqa: E402
import metric_oracle as M  # noqa: E402

PEAK_BPS = 8e12
LEGS = {  # name: (codec, source components, decoded channels)
    "dxt1": (pkg.DXT1, 4, 3), "dxt5": (pkg.DXT5, 4, 4), "etc1": (pkg.ETC1, 3, 3), "pvrtc2": (pkg.PVRTC2, 4, 4),
}


def time_calls(fn, k, reps, precondition_s):
    t0 = time.time()
    while time.time() - t0 < precondition_s:  # untimed: out of idle, into the steady power state
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / k)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--precondition", type=float, default=1.0)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = pkg.lib()
    s, n = a.size, a.n
    bad = False
    for leg in a.legs.split(","):
        codec, comps, dch = LEGS[leg]
        imgs = [T.s_mixed(s, s, comps, index=60 + i) for i in range(2)]  # two contents, alternating over the batch
        src = torch.cat([torch.from_numpy(imgs[i % 2].reshape(-1)) for i in range(n)]).to(dev)
        img_bytes, blk_bytes, pix_bytes = s * s * comps, pkg.encoded_size(codec, s, s), s * s * dch
        blocks = torch.empty((n, blk_bytes), dtype=torch.uint8, device=dev)
        scratch_blocks = torch.empty_like(blocks)
        pixels = torch.empty((n, pix_bytes), dtype=torch.uint8, device=dev)
        stats = torch.empty((n, pkg.ERROR_STATS_BYTES), dtype=torch.uint8, device=dev)
        st = pkg._stream_handle()
        if codec == pkg.PVRTC2:  # its encoder's scratch memory, caller-owned like a streaming caller's
            ws = torch.empty((pkg.pvrtc_workspace_size(s, n),), dtype=torch.uint8, device=dev)
            pkg.pvrtc_set_workspace(ws)

        def encode(dst=scratch_blocks):
            rc = lib.icamd_encode_device(codec, pkg.ETC_HEURISTIC, comps, 0, s, s, s, s, s * comps, n, img_bytes, blk_bytes,
                                         src.data_ptr(), dst.data_ptr(), st)
            assert rc == 0, rc

        def metric():
            rc = lib.icamd_measure_error_device(codec, comps, 0, s, s, s, s, s * comps, n, img_bytes, blk_bytes, src.data_ptr(),
                                                blocks.data_ptr(), stats.data_ptr(), st)
            assert rc == 0, rc

        detour_sse = [None]

        def detour():
            rc = lib.icamd_decode_device(codec, 0, s, s, 0, n, blk_bytes, pix_bytes, blocks.data_ptr(), pixels.data_ptr(), st)
            assert rc == 0, rc
            a_ = src.view(n, s * s, comps)[..., :dch].to(torch.int32)
            d = a_ - pixels.view(n, s * s, dch).to(torch.int32)
            detour_sse[0] = (d * d).sum(dim=1, dtype=torch.int64)

        encode(blocks)
        torch.cuda.synchronize()
        res = {}
        for name, fn in (("metric", metric), ("detour", detour), ("encode", encode)):
            t = time_calls(fn, a.k if name != "detour" else max(2, a.k // 4), a.reps, a.precondition)
            res[name] = (statistics.median(t), min(t), max(t))
        metric()
        detour()
        torch.cuda.synchronize()
        sse, mx = pkg._split_stats(stats)
        parity_detour = bool(torch.equal(sse[:, :dch], detour_sse[0]))
        want = M.measure(codec, imgs[0], blocks[0].cpu().numpy().tobytes(), s, s, comps)
        parity_oracle = bool((sse[0].cpu().numpy() == want[0]).all() and (mx[0].cpu().numpy() == want[1]).all())
        bad |= not (parity_detour and parity_oracle)
        read = n * (img_bytes + blk_bytes)
        rec = {"leg": leg, "kernel": pkg.metric_kernel_name(codec, comps), "n_images": n, "size": s, "src_components": comps,
               "device": torch.cuda.get_device_name(0), "parity_vs_detour": parity_detour, "parity_vs_oracle": parity_oracle,
               "psnr_image0": round(pkg.psnr_from_stats(sse[0, :dch].cpu().numpy(), s * s, dch), 3)}
        for name, (med, lo, hi) in res.items():
            rec[name + "_ms"] = round(med, 4)
            rec[name + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
        rec["metric_alg_GBps"] = round(read / (res["metric"][0] * 1e-3) / 1e9, 1)
        rec["metric_frac_8TBps"] = round(read / (res["metric"][0] * 1e-3) / PEAK_BPS, 3)
        rec["detour_over_metric"] = round(res["detour"][0] / res["metric"][0], 3)
        rec["metric_over_encode"] = round(res["metric"][0] / res["encode"][0], 3)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        if codec == pkg.PVRTC2:
            pkg.pvrtc_set_workspace(None)
        del src, blocks, scratch_blocks, pixels, stats
        detour_sse[0] = None
        torch.cuda.empty_cache()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
