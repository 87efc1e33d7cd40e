#!/usr/bin/env python3
"""Device-resident throughput of the ETC2 RGBA8 encoder (extension, include/ic_amd.h ICAMD_ETC2_RGBA8) against ETC1 from
the same RGBA8 inputs, per strategy.

Legs: for each EtcCompressor strategy, 16 x 4096^2 RGBA8 (1 GiB of source) through ICAMD_ETC2_RGBA8 and, in the same run on
the same buffer, through ICAMD_ETC1 with src_components = 4.  The figure to record is the ratio ETC2 / ETC1 of the median ms
per launch (what the fused EAC alpha search adds to the colour search), plus Gpixel/s of each.
Method (scripts/bench_bc45.py): untimed preconditioning calls, then device events around K back-to-back launches, repeated; the
median and the spread (min / max) of ms per launch are reported.  One JSON line per strategy, with a parity flag: the colour
half of image 0 against the ETC1 kernel's output for it, and the alpha half of its first four block rows against the numpy
definition (tests/etc2_oracle.py: test infrastructure, the checker only).

  python scripts/bench_etc2.py [--k 5] [--reps 5] [--size 4096] [--images 16] [--strategies 0,1,2,3]
Exit status 1 if any leg's parity fails."""
import argparse
import json
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
import etc2_oracle as E  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--content", default="mixed", choices=sorted(B.GENERATORS))
    ap.add_argument("--strategies", default="0,1,2,3")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s, n = a.size, a.images
    img0 = B.image(a.content, s, s, 4, index=1)
    src = torch.from_numpy(img0).to(dev).reshape(1, -1).repeat(n, 1)
    out2 = torch.empty((n, E.encoded_size(s, s)), dtype=torch.uint8, device=dev)
    out1 = torch.empty((n, E.encoded_size(s, s) // 2), dtype=torch.uint8, device=dev)
    strip_rows = min(16, s)
    want_alpha = E.eac_encode(E.block_alphas(img0[:strip_rows, :, 3], strip_rows, s, strip_rows, s))
    bad = False
    for strategy in [int(x) for x in a.strategies.split(",")]:
        f2 = lambda: pkg.encode_device(pkg.ETC2_RGBA8, src, s, s, 4, etc_strategy=strategy, n_images=n, out=out2)  # noqa: E731
        f1 = lambda: pkg.encode_device(pkg.ETC1, src, s, s, 4, etc_strategy=strategy, n_images=n, out=out1)  # noqa: E731
        ms2 = time_launches(f2, a.k, a.reps, a.warmup)
        ms1 = time_launches(f1, a.k, a.reps, a.warmup)
        torch.cuda.synchronize()
        got2 = out2[0].cpu().numpy().reshape(-1, 16)
        ok = bool((got2[:, 8:] == out1[0].cpu().numpy().reshape(-1, 8)).all()) and \
            bool((got2[:want_alpha.shape[0], :8] == want_alpha).all())
        bad |= not ok
        m2, m1 = statistics.median(ms2), statistics.median(ms1)
        print(json.dumps({
            "strategy": NAMES.get(strategy, str(strategy)), "images": n, "size": s, "content": a.content,
            "etc2_ms_per_launch_median": round(m2, 4), "etc2_ms_min": round(min(ms2), 4), "etc2_ms_max": round(max(ms2), 4),
            "etc1_ms_per_launch_median": round(m1, 4), "etc1_ms_min": round(min(ms1), 4), "etc1_ms_max": round(max(ms1), 4),
            "ratio_etc2_over_etc1": round(m2 / m1, 3),
            "etc2_gpixels_per_s": round(n * s * s / (m2 * 1e-3) / 1e9, 2), "etc1_gpixels_per_s": round(n * s * s / (m1 * 1e-3) / 1e9, 2),
            "parity": "colour half = ETC1 kernel, alpha half = definition (image 0)" if ok else "MISMATCH"}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
