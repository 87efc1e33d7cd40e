#!/usr/bin/env python3
"""Device-resident throughput and quality of the ETC2 RGB8 punch-through alpha encoder (extension, include/ic_amd.h
ICAMD_ETC2_RGB8A1) next to ICAMD_ETC2_RGB8 from RGBA8 and ICAMD_ETC2_RGBA8 from the same buffer in the same run,
per strategy and per content.

Contents, 16 x 4096^2 RGBA8: "gradient", "smooth" and "mixed" with alpha 255 everywhere (the noise-free ramp, on which no wave
needs the differential search; the smooth generator with its noise and wrap-around seams; the quadrant mix, whose noise gives
individual ETC1 words), and "cutout": the mixed colour under a blobby alpha mask (discs with soft rims, a 256 x 256 tile repeated).
Reported per leg: the median ms per launch of the three codecs and their run-to-run spread (min / max over the repetitions),
the ratios A1 / RGB8 and A1 / RGBA8, the share of blocks of image 0 per class -- E kept (the ETC1 word), D opaque (E individual:
the differential search in its place), planar, D masked (1..15 transparent texels), all transparent -- and the PSNR over R, G, B
of all three and over R, G, B, A of A1 and RGBA8 from icamd_measure_error_device (for A1 the colour under a transparent texel
counts against the decoded 0, as include/ic_amd.h states).
Method: untimed preconditioning calls of every codec, then device events around K back-to-back launches, repeated, the three
codecs alternating within every repetition.
Checks, per leg: the first four block rows of image 0 equal the numpy statement (tests/etc2_a1_oracle.py: test infrastructure,
the checker only), every fully opaque block is the ETC1 word, a planar word or a differential word with Op = 1, and decoded
alpha is the source's mask.

  python scripts/bench_etc2_a1.py [--k 5] [--reps 5] [--size 4096] [--images 16] [--strategies 0,1,2,3]
                                  [--contents gradient,smooth,mixed,cutout] > profiles/etc2_a1_bench.jsonl
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
import etc2_a1_oracle as A  # noqa: E402
import etc2_colour_oracle as C  # noqa: E402

NAMES = {0: "split_h", 1: "split_v", 2: "smaller_error", 3: "heuristic"}


def time_launches(fns, k, reps, warmup):
    """{name: fn} -> {name: [ms per launch, one per repetition]}; the codecs alternate within every repetition, so that a drift of
    the machine meets all of them alike."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) / k)
    return out


def psnr(sse, n_values):
    return round(10.0 * math.log10(255.0 * 255.0 * n_values / sse), 2) if sse else float("inf")


def content_image(content, s):
    # ("gradient": the noise-free ramp of tests/etc2_colour_oracle.py; the "smooth" generator carries 5 bits of noise and wraps)
    img = C.gradient(s, s, 4) if content == "gradient" else B.image("smooth" if content == "smooth" else "mixed", s, s, 4, index=1).copy()
    if content == "cutout":
        tile = A.alpha_blobs(min(s, 256), min(s, 256), index=1)
        reps = (s + tile.shape[0] - 1) // tile.shape[0]
        img[..., 3] = np.tile(tile, (reps, reps))[:s, :s]
    else:
        img[..., 3] = 255
    return img


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--contents", default="gradient,smooth,mixed,cutout")
    ap.add_argument("--strategies", default="0,1,2,3")
    a = ap.parse_args()
    if a.size % 4:
        ap.error("--size must be a multiple of 4")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s, n = a.size, a.images
    per = A.encoded_size(s, s)
    out_a1 = torch.empty((n, per), dtype=torch.uint8, device=dev)
    out_rgb = torch.empty((n, per), dtype=torch.uint8, device=dev)
    out_etc1 = torch.empty((n, per), dtype=torch.uint8, device=dev)
    out_rgba = torch.empty((n, 2 * per), dtype=torch.uint8, device=dev)
    strip_rows = min(16, s)
    bad = False
    for content in [c for c in a.contents.split(",") if c]:
        img0 = content_image(content, s)
        src = torch.from_numpy(img0).to(dev).reshape(1, -1).repeat(n, 1)
        n_opq = (img0[..., 3] >= 128).reshape(s // 4, 4, s // 4, 4).sum(axis=(1, 3)).reshape(-1)  # (the size is a multiple of 4)
        full, clear = n_opq == 16, n_opq == 0
        for strategy in [int(x) for x in a.strategies.split(",")]:
            legs = {"a1": lambda: pkg.encode_device(pkg.ETC2_RGB8A1, src, s, s, 4, etc_strategy=strategy, n_images=n, out=out_a1),
                    "rgb8": lambda: pkg.encode_device(pkg.ETC2_RGB8, src, s, s, 4, etc_strategy=strategy, n_images=n, out=out_rgb),
                    "rgba8": lambda: pkg.encode_device(pkg.ETC2_RGBA8, src, s, s, 4, etc_strategy=strategy, n_images=n, out=out_rgba)}
            ms = time_launches(legs, a.k, a.reps, a.warmup)
            pkg.encode_device(pkg.ETC1, src, s, s, 4, etc_strategy=strategy, n_images=n, out=out_etc1)
            sse_a1, _ = pkg.measure_error_device(pkg.ETC2_RGB8A1, src, out_a1.reshape(-1), s, s, 4, n_images=n)
            sse_rgb, _ = pkg.measure_error_device(pkg.ETC2_RGB8, src, out_rgb.reshape(-1), s, s, 4, n_images=n)
            sse_rgba, _ = pkg.measure_error_device(pkg.ETC2_RGBA8, src, out_rgba.reshape(-1), s, s, 4, n_images=n)
            torch.cuda.synchronize()
            got, e = out_a1[0].cpu().numpy().reshape(-1, 8), out_etc1[0].cpu().numpy().reshape(-1, 8)
            kept = full & (got == e).all(axis=1)
            planar = full & ~kept & (A.modes(got) == A.PLANAR)
            d_opaque = full & ~kept & ~planar
            shares = {"e_kept": kept.mean(), "d_opaque": d_opaque.mean(), "planar": planar.mean(),
                      "d_masked": (~full & ~clear).mean(), "all_transparent": clear.mean()}
            want = A.oracle_encode(img0[:strip_rows], strip_rows, s, 0, strategy)
            strip = A.decode_blocks(got[:len(want) // 8])[..., 3]
            mask = A.block_texels(img0[:strip_rows], strip_rows, s, strip_rows, s)[..., 3] >= 128
            ok = got[:len(want) // 8].tobytes() == want and bool((strip == np.where(mask, 255, 0)).all()) and \
                bool(((e[d_opaque][:, 3] & 2) == 0).all()) and bool((A.opaque_bit(got[d_opaque]) == 1).all()) and \
                bool((got[clear] == np.frombuffer(A.ALL_TRANSPARENT, np.uint8)).all())
            bad |= not ok
            med = {name: statistics.median(v) for name, v in ms.items()}
            a1, rgb, rgba = (sse[0].cpu().numpy() for sse in (sse_a1, sse_rgb, sse_rgba))
            print(json.dumps({
                "content": content, "strategy": NAMES.get(strategy, str(strategy)), "images": n, "size": s,
                "etc2_a1_ms": spread(ms["a1"]), "etc2_rgb8_ms": spread(ms["rgb8"]), "etc2_rgba8_ms": spread(ms["rgba8"]),
                "ratio_a1_over_rgb8": round(med["a1"] / med["rgb8"], 3), "ratio_a1_over_rgba8": round(med["a1"] / med["rgba8"], 3),
                "etc2_a1_gpixels_per_s": round(n * s * s / (med["a1"] * 1e-3) / 1e9, 2),
                "class_shares": {k: round(float(v), 4) for k, v in shares.items()},
                "psnr_rgb_db": {"a1": psnr(int(a1[:3].sum()), 3 * s * s), "rgb8": psnr(int(rgb[:3].sum()), 3 * s * s),
                                "rgba8": psnr(int(rgba[:3].sum()), 3 * s * s)},
                "psnr_rgba_db": {"a1": psnr(int(a1.sum()), 4 * s * s), "rgba8": psnr(int(rgba.sum()), 4 * s * s)},
                "check": "first rows = statement, alpha = mask, classes consistent (image 0)" if ok else "MISMATCH"}), flush=True)
        del src
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
