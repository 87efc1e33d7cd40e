#!/usr/bin/env python3
"""Device-resident throughput and quality of the 16-bit EAC R11 / RG11 encoders (extension, include/ic_amd.h
icamd_encode_eac11_16_device), next to the route a 16-bit source had to take before -- source >> 8, then
icamd_encode_device(ICAMD_EAC_R11) from R8 -- in the same run.

Per content (ramp: a smooth two-channel ramp; noise: uniform 16-bit noise) at 16 x 4096^2:
  r11<-r16, rg11<-rg16, signed_r11<-r16   the new encoders (the signed leg reads the same samples minus 32768);
  r11<-r8 (existing route)                icamd_encode_device(ICAMD_EAC_R11) on the top bytes of the R16 plane.
Every leg reports ms per launch (median, min, max), the 16-bit PSNR of image 0 (peak 65535, signed 32767) from
icamd_measure_error_eac11_16_device against the 16-bit source, and the share of image 0's words with multiplier 0.  One line
compares the medians of r11<-r16 and the existing route.  Parity: the first block row of image 0 against the numpy definition
(tests/eac11_16_oracle.py: test infrastructure, the checker only).
Method (scripts/bench_eac11.py): untimed preconditioning calls, then device events around K back-to-back launches, repeated.

  python scripts/bench_eac11_16.py [--k 5] [--reps 5] [--size 4096] [--images 16]
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
import eac11_16_oracle as A  # noqa: E402
import eac11_oracle as A8  # noqa: E402


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


def content(name, s):
    """(s, s, 2) uint16"""
    y, x = np.mgrid[0:s, 0:s]
    if name == "ramp":  # slopes that keep 4096 pixels inside the range
        return np.stack([20000 + 5 * x + 3 * y, 60000 - 4 * x - 2 * y], axis=-1).astype(np.uint16)
    return np.random.Generator(np.random.PCG64(4116)).integers(0, 65536, (s, s, 2), dtype=np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--images", type=int, default=16)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s, n = a.size, a.images
    strip = min(4, s)
    bad = False
    for name in ("ramp", "noise"):
        img = content(name, s)
        r16 = np.ascontiguousarray(img[..., 0])
        legs = [
            ("r11<-r16", A.EAC_R11, 1, r16),
            ("rg11<-rg16", A.EAC_RG11, 2, img),
            ("signed_r11<-r16", A.EAC_SIGNED_R11, 1, (r16.astype(np.int32) - 32768).astype(np.int16)),
        ]
        medians = {}
        for leg, codec, chans, src in legs:
            d1 = torch.from_numpy(src.reshape(-1).view(np.uint8).copy()).to(dev)
            d = d1.reshape(1, -1).repeat(n, 1)
            out = torch.empty((n, A.encoded_size(codec, s, s)), dtype=torch.uint8, device=dev)
            ms = time_launches(lambda: pkg.encode_eac11_16_device(codec, d, s, s, chans, n_images=n, out=out), a.k, a.reps, a.warmup)
            sse, _ = pkg.measure_error_eac11_16_device(codec, d1, out[0], s, s, chans)
            torch.cuda.synchronize()
            got = out[0].cpu().numpy()
            want = A.oracle_encode(codec, src.reshape(s, s, chans)[:strip], strip, s, chans)
            ok = got[:len(want)].tobytes() == want
            bad |= not ok
            k = A.comps_out(codec)
            medians[leg] = statistics.median(ms)
            print(json.dumps({"leg": leg, "content": name, "images": n, "size": s, "ms_per_launch_median": round(medians[leg], 4),
                              "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                              "gpixels_per_s": round(n * s * s / (medians[leg] * 1e-3) / 1e9, 2),
                              "psnr16_db": round(pkg.psnr16_from_stats(sse[0].cpu().numpy(), s * s, k, A.is_signed(codec)), 2),
                              "multiplier0_share": round(float(((got.reshape(-1, 8)[:, 1] >> 4) == 0).mean()), 4),
                              "kernel": pkg.eac11_16_kernel_name(codec, chans),
                              "parity": "definition (image 0, first block row)" if ok else "MISMATCH"}), flush=True)
        # the existing route: the top bytes through the 8-bit encoder, its words decoded to 16 bits
        r8 = (r16 >> 8).astype(np.uint8)
        d8 = torch.from_numpy(r8.reshape(-1)).to(dev).reshape(1, -1).repeat(n, 1)
        out = torch.empty((n, A.encoded_size(A.EAC_R11, s, s)), dtype=torch.uint8, device=dev)
        ms = time_launches(lambda: pkg.encode_device(pkg.EAC_R11, d8, s, s, 1, n_images=n, out=out), a.k, a.reps, a.warmup)
        d16 = torch.from_numpy(r16.reshape(-1).view(np.uint8).copy()).to(dev)
        sse, _ = pkg.measure_error_eac11_16_device(A.EAC_R11, d16, out[0], s, s, 1)
        torch.cuda.synchronize()
        got = out[0].cpu().numpy()
        ok = got[:s // 4 * 8].tobytes() == A8.channel_words(r8[:strip], strip, s).tobytes()
        bad |= not ok
        m = statistics.median(ms)
        print(json.dumps({"leg": "r11<-r8 (existing route)", "content": name, "images": n, "size": s,
                          "ms_per_launch_median": round(m, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                          "gpixels_per_s": round(n * s * s / (m * 1e-3) / 1e9, 2),
                          "psnr16_db": round(pkg.psnr16_from_stats(sse[0].cpu().numpy(), s * s, 1), 2),
                          "multiplier0_share": round(float(((got.reshape(-1, 8)[:, 1] >> 4) == 0).mean()), 4),
                          "kernel": pkg.kernel_name(pkg.EAC_R11, 1),
                          "parity": "definition (image 0, first block row)" if ok else "MISMATCH"}), flush=True)
        print(json.dumps({"comparison": "r11<-r16 / r11<-r8", "content": name,
                          "ratio_of_medians": round(medians["r11<-r16"] / m, 3)}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
