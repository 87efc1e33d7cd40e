#!/usr/bin/env python3
"""Device-resident throughput of the BC4 / BC5 (RGTC) encoders and decoders (extension, include/ic_amd.h ICAMD_BC4).

Legs (every encode leg reads 1 GiB of source, as the headline does):
  bc4 <- r8     64 x 4096^2      bc5 <- rg8    32 x 4096^2      bc5 <- rgba8  16 x 4096^2
  bc4 -> r8     64 x 4096^2      bc5 -> rg8    32 x 4096^2
Method (scripts/bench_next_rows.py): untimed preconditioning calls, then device events around K back-to-back launches,
repeated; the median and the spread (min / max) of ms per launch are reported.  One JSON line per leg: ms per launch, Mpixels/s,
algorithmic bytes (source read + result written, once each) and their fraction of 8 TB/s, and a parity flag -- image 0 of the
last timed output against the definition computed with the oracle's DXT5 (tests/bc45_oracle.py: test infrastructure, the
checker only).

  python scripts/bench_bc45.py [--k 20] [--reps 7] [--size 4096] [--legs bc4_r8,bc5_rg8,...]
Exit status 1 if any leg's parity fails."""
import argparse
import ctypes
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

PEAK_BPS = 8e12


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
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--legs", default="bc4_r8,bc5_rg8,bc5_rgba8,bc4_decode,bc5_decode")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s = a.size
    bad = False
    for leg in a.legs.split(","):
        codec = B.BC5 if leg.startswith("bc5") else B.BC4
        decode = leg.endswith("decode")
        comps = 1 if leg == "bc4_r8" else 2 if leg == "bc5_rg8" else 4 if leg == "bc5_rgba8" else B.comps_out(codec)
        n = (64 if codec == B.BC4 else 32) if decode else (1 << 30) // (s * s * comps)
        per = B.encoded_size(codec, s, s)
        img0 = B.image("mixed", s, s, 4, index=1)[..., :comps].copy()
        if decode:
            blocks0 = B.oracle_encode(codec, img0, s, s, comps)
            src = torch.from_numpy(np.frombuffer(blocks0, np.uint8)).to(dev).repeat(n)
            out = torch.empty((n, s * s * comps), dtype=torch.uint8, device=dev)
            src_p, out_p = ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(out.data_ptr())
            # the C entry point itself: decode_device would add a zero fill of the output to every call
            fn = lambda: pkg.lib().icamd_decode_device(codec, 0, s, s, 0, n, per, s * s * comps, src_p, out_p,  # noqa: E731
                                                      pkg._stream_handle())
            want = B.oracle_decode(codec, blocks0, s, s).tobytes()
            read, written = n * per, n * s * s * comps
        else:
            src = torch.from_numpy(img0).to(dev).reshape(1, -1).repeat(n, 1)
            out = torch.empty((n, per), dtype=torch.uint8, device=dev)
            fn = lambda: pkg.encode_device(codec, src, s, s, comps, n_images=n, out=out)  # noqa: E731
            want = B.oracle_encode(codec, img0, s, s, comps)
            read, written = n * s * s * comps, n * per
        ms = time_launches(fn, a.k, a.reps, a.warmup)
        torch.cuda.synchronize()
        ok = out[0].cpu().numpy().tobytes() == want
        bad |= not ok
        med = statistics.median(ms)
        gbps = (read + written) / (med * 1e-3) / 1e9
        print(json.dumps({
            "leg": leg, "codec": "bc5" if codec == B.BC5 else "bc4", "images": n, "size": s, "src_components": comps,
            "direction": "decode" if decode else "encode",
            "kernel": ("icamd_bc5_decode_kernel" if codec == B.BC5 else "icamd_bc4_decode_kernel") if decode
            else pkg.kernel_name(codec, comps),
            "ms_per_launch_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "spread_pct": round(100.0 * (max(ms) - min(ms)) / med, 2),
            "mpixels_per_s": round(n * s * s / (med * 1e-3) / 1e6, 1),
            "algorithmic_bytes": read + written, "algorithmic_GBps": round(gbps, 1), "frac_of_8TBps": round(gbps * 1e9 / PEAK_BPS, 4),
            "parity": "bit-exact vs oracle definition (image 0)" if ok else "MISMATCH"}), flush=True)
        del src, out
        torch.cuda.empty_cache()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
