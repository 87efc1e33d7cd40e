#!/usr/bin/env python3
"""Device-resident throughput of the EAC R11 / RG11 encoders and decoders (extension, include/ic_amd.h ICAMD_EAC_R11), next to
ICAMD_ETC2_RGBA8 kSplitHorizontally on the same RGBA8 buffer in the same run.

Legs at 16 x 4096^2: R11 <- R8, R11 <- RGBA8, RG11 <- RG8, RG11 <- RGBA8, both decoders, and ETC2 RGBA8 (kSplitHorizontally) from
the RGBA8 buffer the R11 / RG11 <- RGBA8 legs read.  Two comparisons follow from work counts alone:
  1. R11 <- RGBA8 takes no longer than ETC2 RGBA8 kSplitHorizontally (same reads, same search, no colour encode, half the store);
  2. RG11 <- RGBA8 takes no more than twice R11 <- RGBA8 (two searches on one read).
They compare medians; where the two legs' min..max intervals overlap the verdict is "tie".
Method (scripts/bench_etc2.py): untimed preconditioning calls, then device events around K back-to-back launches, repeated; the
median and the spread (min / max) of ms per launch are reported.  One JSON line per leg with a parity flag -- the first four
block rows of image 0 against the numpy definition (tests/eac11_oracle.py: test infrastructure, the checker only) -- and one
line per comparison.

  python scripts/bench_eac11.py [--k 5] [--reps 5] [--size 4096] [--images 16] [--content mixed|noise|smooth|flat|saturated]
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
import eac11_oracle as A  # noqa: E402
import etc2_oracle as E  # noqa: E402


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


def verdict(ms_a, ms_b, factor):
    """ms_a against factor * ms_b: "pass" / "fail" on the medians, "tie" where the min..max intervals overlap."""
    lo_b, hi_b = factor * min(ms_b), factor * max(ms_b)
    if min(ms_a) <= hi_b and lo_b <= max(ms_a):
        return "tie"
    return "pass" if statistics.median(ms_a) <= factor * statistics.median(ms_b) else "fail"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--content", default="mixed", choices=sorted(B.GENERATORS))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s, n = a.size, a.images
    img0 = B.image(a.content, s, s, 4, index=1)
    strip = min(16, s)
    words = [A.channel_words(img0[:strip, :, c], strip, s) for c in (0, 1)]  # the first four block rows of R and of G
    want = {A.EAC_R11: words[0], A.EAC_RG11: np.concatenate(words, axis=1)}
    want_alpha = E.eac_encode(E.block_alphas(img0[:strip, :, 3], strip, s, strip, s))
    srcs = {c: torch.from_numpy(np.ascontiguousarray(img0[..., :c])).to(dev).reshape(1, -1).repeat(n, 1) for c in (1, 2, 4)}
    results, bad = {}, False

    def report(leg, ms, ok, **extra):
        nonlocal bad
        bad |= not ok
        m = statistics.median(ms)
        results[leg] = ms
        print(json.dumps(dict({"leg": leg, "images": n, "size": s, "content": a.content, "ms_per_launch_median": round(m, 4),
                               "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                               "gpixels_per_s": round(n * s * s / (m * 1e-3) / 1e9, 2), "parity": "definition (image 0)" if ok else "MISMATCH"},
                              **extra)), flush=True)

    blocks = {}
    for codec, comps, leg in ((A.EAC_R11, 1, "r11<-r8"), (A.EAC_R11, 4, "r11<-rgba8"), (A.EAC_RG11, 2, "rg11<-rg8"),
                              (A.EAC_RG11, 4, "rg11<-rgba8")):
        out = torch.empty((n, A.encoded_size(codec, s, s)), dtype=torch.uint8, device=dev)
        ms = time_launches(lambda: pkg.encode_device(codec, srcs[comps], s, s, comps, n_images=n, out=out), a.k, a.reps, a.warmup)
        torch.cuda.synchronize()
        got = out[0].cpu().numpy().reshape(-1, A.block_bytes(codec))
        report(leg, ms, bool((got[:want[codec].shape[0]] == want[codec]).all()), kernel=pkg.kernel_name(codec, comps))
        blocks[codec] = out
    out2 = torch.empty((n, E.encoded_size(s, s)), dtype=torch.uint8, device=dev)
    ms = time_launches(lambda: pkg.encode_device(pkg.ETC2_RGBA8, srcs[4], s, s, 4, etc_strategy=pkg.ETC_SPLIT_HORIZONTALLY,
                                                 n_images=n, out=out2), a.k, a.reps, a.warmup)
    torch.cuda.synchronize()
    got = out2[0].cpu().numpy().reshape(-1, 16)
    report("etc2_rgba8_split_h<-rgba8", ms, bool((got[:want_alpha.shape[0], :8] == want_alpha).all()),
           kernel="icamd_etc2_rgba8_split_h_kernel")
    for codec, leg in ((A.EAC_R11, "r11_decode"), (A.EAC_RG11, "rg11_decode")):
        k = A.comps_out(codec)
        got = torch.zeros((n, s * s * k), dtype=torch.uint8, device=dev)
        src_p, out_p, per = ctypes.c_void_p(blocks[codec].data_ptr()), ctypes.c_void_p(got.data_ptr()), blocks[codec].shape[1]
        # the C entry point itself: decode_device would add a zero fill of the output to every call
        ms = time_launches(lambda: pkg.lib().icamd_decode_device(codec, 0, s, s, 0, n, per, s * s * k, src_p, out_p, None),
                           a.k, a.reps, a.warmup)
        torch.cuda.synchronize()
        rows = got[0].cpu().numpy().reshape(s, s * k)[:strip]
        report(leg, ms, rows.tobytes() == A.oracle_decode(codec, want[codec].tobytes(), strip, s).tobytes(),
               kernel="icamd_eac_rg11_decode_kernel" if codec == A.EAC_RG11 else "icamd_eac_r11_decode_kernel")
    for name, x, y, factor in (("r11<-rgba8 <= etc2_rgba8_split_h", "r11<-rgba8", "etc2_rgba8_split_h<-rgba8", 1.0),
                               ("rg11<-rgba8 <= 2 x r11<-rgba8", "rg11<-rgba8", "r11<-rgba8", 2.0)):
        print(json.dumps({"comparison": name, "content": a.content, "verdict": verdict(results[x], results[y], factor),
                          "ratio_of_medians": round(statistics.median(results[x]) / statistics.median(results[y]), 3)}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
