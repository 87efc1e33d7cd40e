#!/usr/bin/env python3
"""Device-resident cost and gain of the T / H pass of ETC2 RGB8 (extension, include/ic_amd.h icamd_encode_etc2_device,
ICAMD_ETC2_MODES_TH) against the default encode of the same buffer in the same run, per content.

Legs: for each content (noise, smooth, edge: the 64 x 64 edge fixture of tests/etc2_th_oracle.py tiled, with +-6 noise per
pixel), 16 x 4096^2 pixels through etc2_modes 1 (the ETC2 RGB8 kernel, then the T / H kernel) and through etc2_modes 0 (the
ETC2 RGB8 kernel alone).  Reported per leg: the median ms per call of both and their spread (min / max), their ratio, the share
of image 0's blocks that became T or H, and the PSNR of both over the three channels from icamd_measure_error_device.
Method (scripts/bench_etc2_rgb8.py): untimed preconditioning calls, then device events around K back-to-back calls, repeated.
Checks, per leg: every block of image 0 that differs from the default encode is a T or H word, the summed squared error does
not exceed the default's, and the first four block rows equal the numpy definition (tests/etc2_th_oracle.py: test
infrastructure, the checker only).

  python scripts/bench_etc2_th.py [--k 5] [--reps 5] [--size 4096] [--images 16] [--comps 4] [--strategy 2]
                                  [--contents noise,smooth,edge]
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
import etc2_th_oracle as H  # noqa: E402


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


def edge_image(s, comps):
    reps = (s + 63) // 64
    base = np.tile(H.edges(0)[..., :3].astype(np.int64), (reps, reps, 1))[:s, :s]
    g = np.random.Generator(np.random.PCG64(9740))
    img = np.full((s, s, comps), 255, np.uint8)
    img[..., :3] = np.clip(base + g.integers(-6, 7, base.shape), 0, 255)
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--comps", type=int, default=4, choices=(3, 4))
    ap.add_argument("--strategy", type=int, default=2)
    ap.add_argument("--contents", default="noise,smooth,edge")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s, n, comps, strategy = a.size, a.images, a.comps, a.strategy
    per = C.encoded_size(s, s)
    out1 = torch.empty((n, per), dtype=torch.uint8, device=dev)
    out0 = torch.empty((n, per), dtype=torch.uint8, device=dev)
    strip_rows = min(16, s)
    bad = False
    for content in [c for c in a.contents.split(",") if c]:
        img0 = edge_image(s, comps) if content == "edge" else B.image(content, s, s, comps, index=1)
        img0 = np.ascontiguousarray(img0).reshape(s, s, comps)
        src = torch.from_numpy(img0).to(dev).reshape(1, -1).repeat(n, 1)
        f1 = lambda: pkg.encode_device(pkg.ETC2_RGB8, src, s, s, comps, etc_strategy=strategy, n_images=n, out=out1,  # noqa: E731
                                       etc2_modes=pkg.ETC2_MODES_TH)
        f0 = lambda: pkg.encode_device(pkg.ETC2_RGB8, src, s, s, comps, etc_strategy=strategy, n_images=n, out=out0)  # noqa: E731
        ms1 = time_launches(f1, a.k, a.reps, a.warmup)
        ms0 = time_launches(f0, a.k, a.reps, a.warmup)
        sse1, _ = pkg.measure_error_device(pkg.ETC2_RGB8, src, out1.reshape(-1), s, s, comps, n_images=n)
        sse0, _ = pkg.measure_error_device(pkg.ETC2_RGB8, src, out0.reshape(-1), s, s, comps, n_images=n)
        torch.cuda.synchronize()
        got1, got0 = out1[0].cpu().numpy().reshape(-1, 8), out0[0].cpu().numpy().reshape(-1, 8)
        same = (got1 == got0).all(axis=1)
        e1, e0 = int(sse1[0, :3].sum().item()), int(sse0[0, :3].sum().item())
        want = H.oracle_encode(img0[:strip_rows], strip_rows, s, comps, 0, strategy)
        m = C.modes(got1[~same])
        ok = bool(((m == C.T_MODE) | (m == C.H_MODE)).all()) and e1 <= e0 and got1[:len(want) // 8].tobytes() == want
        bad |= not ok
        m1, m0 = statistics.median(ms1), statistics.median(ms0)
        print(json.dumps({
            "content": content, "strategy": strategy, "images": n, "size": s, "src_components": comps,
            "modes_th_ms_per_call_median": round(m1, 4), "modes_th_ms_min": round(min(ms1), 4), "modes_th_ms_max": round(max(ms1), 4),
            "modes_default_ms_per_call_median": round(m0, 4), "modes_default_ms_min": round(min(ms0), 4),
            "modes_default_ms_max": round(max(ms0), 4), "ratio_th_over_default": round(m1 / m0, 3),
            "th_pass_ms": round(m1 - m0, 4), "modes_th_gpixels_per_s": round(n * s * s / (m1 * 1e-3) / 1e9, 2),
            "th_share": round(float((~same).mean()), 4),
            "psnr_rgb_modes_th_db": psnr(e1, 3 * s * s), "psnr_rgb_modes_default_db": psnr(e0, 3 * s * s),
            "check": "changed blocks are T / H words, sse <= default, first rows = definition (image 0)" if ok else "MISMATCH"}),
            flush=True)
        del src
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
