#!/usr/bin/env python3
"""Device-resident throughput and quality of the ETC2 RGB8 encoder (extension, include/ic_amd.h ICAMD_ETC2_RGB8)
against ETC1 from the same buffer in the same run, per strategy and per content generator.

Legs: for each content generator (gradient, smooth, mixed, noise) and each EtcCompressor strategy, 16 x 4096^2 pixels through
ICAMD_ETC2_RGB8 and through ICAMD_ETC1.  Reported per leg: the median ms per launch of both and their spread (min / max), the
ratio ETC2 RGB8 / ETC1 (what the planar candidate and the choice add to the ETC1 search), the share of planar blocks in image
0, and the PSNR of both over the three channels from icamd_measure_error_device.
Method (scripts/bench_etc2.py): untimed preconditioning calls, then device events around K back-to-back launches, repeated.
Checks, per leg: every block of image 0 is either the ETC1 kernel's word or a planar word, the summed squared error does not
exceed ETC1's, and the first four block rows equal the numpy definition (tests/etc2_colour_oracle.py: test infrastructure,
the checker only).

--decode adds one leg: icamd_decode_device(ICAMD_ETC2_RGBA8) on encoder-written blocks of the mixed content (the blocks the
library itself writes: ETC1-compatible colour words), median and spread of ms per launch.

  python scripts/bench_etc2_rgb8.py [--k 5] [--reps 5] [--size 4096] [--images 16] [--comps 4] [--strategies 0,1,2,3]
                                    [--contents gradient,smooth,mixed,noise] [--decode]
Exit status 1 if any leg's check fails."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ic_amd_loader  # noqa: E402

pkg = ic_amd_loader.load_package()
import bc45_oracle as B  # noqa: E402
import etc2_colour_oracle as C  # noqa: E402

NAMES = {0: "split_h", 1: "split_v", 2: "smaller_error", 3: "heuristic"}


def time_launches(fn, k, reps, warmup):
    for _ in range(warmup):
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


def psnr(sse_rgb, n_values):
    return round(10.0 * math.log10(255.0 * 255.0 * n_values / sse_rgb), 2) if sse_rgb else float("inf")


def decode_leg(a, dev):
    s, n = a.size, a.images
    img0 = B.image("mixed", s, s, 4, index=1)
    src = torch.from_numpy(img0).to(dev).reshape(1, -1).repeat(n, 1)
    blocks = pkg.encode_device(pkg.ETC2_RGBA8, src, s, s, 4, etc_strategy=3, n_images=n)
    torch.cuda.synchronize()
    del src
    ms = time_launches(lambda: pkg.decode_device(pkg.ETC2_RGBA8, blocks.reshape(-1), s, s, n_images=n), a.k, a.reps, a.warmup)
    print(json.dumps({"leg": "decode_etc2_rgba8_encoder_written", "images": n, "size": s, "ms_per_launch_median": round(statistics.median(ms), 4),
                      "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "ms_all": [round(x, 4) for x in ms]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--comps", type=int, default=4, choices=(3, 4))
    ap.add_argument("--contents", default="gradient,smooth,mixed,noise")
    ap.add_argument("--strategies", default="0,1,2,3")
    ap.add_argument("--decode", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s, n, comps = a.size, a.images, a.comps
    per = C.encoded_size(s, s)
    out2 = torch.empty((n, per), dtype=torch.uint8, device=dev)
    out1 = torch.empty((n, per), dtype=torch.uint8, device=dev)
    strip_rows = min(16, s)
    bad = False
    for content in [c for c in a.contents.split(",") if c]:
        # ("gradient": the noise-free ramp of tests/etc2_colour_oracle.py; the "smooth" generator carries 5 bits of noise)
        img0 = C.gradient(s, s, comps) if content == "gradient" else B.image(content, s, s, comps, index=1)
        src = torch.from_numpy(img0).to(dev).reshape(1, -1).repeat(n, 1)
        for strategy in [int(x) for x in a.strategies.split(",")]:
            f2 = lambda: pkg.encode_device(pkg.ETC2_RGB8, src, s, s, comps, etc_strategy=strategy, n_images=n, out=out2)  # noqa: E731
            f1 = lambda: pkg.encode_device(pkg.ETC1, src, s, s, comps, etc_strategy=strategy, n_images=n, out=out1)  # noqa: E731
            ms2 = time_launches(f2, a.k, a.reps, a.warmup)
            ms1 = time_launches(f1, a.k, a.reps, a.warmup)
            sse2, _ = pkg.measure_error_device(pkg.ETC2_RGB8, src, out2.reshape(-1), s, s, comps, n_images=n)
            sse1, _ = pkg.measure_error_device(pkg.ETC1, src, out1.reshape(-1), s, s, comps, n_images=n)
            torch.cuda.synchronize()
            got2, got1 = out2[0].cpu().numpy().reshape(-1, 8), out1[0].cpu().numpy().reshape(-1, 8)
            same = (got2 == got1).all(axis=1)
            e2, e1 = int(sse2[0, :3].sum().item()), int(sse1[0, :3].sum().item())
            want = C.oracle_encode(img0[:strip_rows], strip_rows, s, comps, 0, strategy)
            ok = bool((C.modes(got2[~same]) == C.PLANAR).all()) and e2 <= e1 and got2[:len(want) // 8].tobytes() == want
            bad |= not ok
            m2, m1 = statistics.median(ms2), statistics.median(ms1)
            print(json.dumps({
                "content": content, "strategy": NAMES.get(strategy, str(strategy)), "images": n, "size": s, "src_components": comps,
                "etc2_rgb8_ms_per_launch_median": round(m2, 4), "etc2_rgb8_ms_min": round(min(ms2), 4), "etc2_rgb8_ms_max": round(max(ms2), 4),
                "etc1_ms_per_launch_median": round(m1, 4), "etc1_ms_min": round(min(ms1), 4), "etc1_ms_max": round(max(ms1), 4),
                "ratio_etc2_rgb8_over_etc1": round(m2 / m1, 3),
                "etc2_rgb8_gpixels_per_s": round(n * s * s / (m2 * 1e-3) / 1e9, 2), "etc1_gpixels_per_s": round(n * s * s / (m1 * 1e-3) / 1e9, 2),
                "planar_share": round(float((~same).mean()), 4),
                "psnr_rgb_etc2_rgb8_db": psnr(e2, 3 * s * s), "psnr_rgb_etc1_db": psnr(e1, 3 * s * s),
                "check": "ETC1 word or planar word, sse <= ETC1, first rows = definition (image 0)" if ok else "MISMATCH"}), flush=True)
        del src
    if a.decode:
        decode_leg(a, dev)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
