#!/usr/bin/env python3
"""Device-resident cost and gain of the colour-mode passes of icamd_encode_etc2_colour_device (extension, include/ic_amd.h;
DESIGN.md 3.19) for ETC2 RGBA8 and ETC2 RGB8A1, against ETC2_COLOUR_DEFAULT of the same buffer in the same run, per content.

Legs: for each codec and content (noise, smooth, edge: the 64 x 64 edge fixture of tests/etc2_th_oracle.py tiled, with +-6
noise per pixel; for ETC2 RGB8A1 also edge_blobs: the edge content under the tiled alpha_blobs mask of tests/etc2_a1_oracle.py;
alpha is 255 everywhere else), 16 x 4096^2 RGBA8 pixels through colour_modes 0, 1 and 2.  Reported per leg: the median ms per call
of each mode and its spread (min / max), the ratio to DEFAULT, the shares of image 0's blocks that are planar, T and H words
(ETC2 RGB8A1: also by block class -- all transparent, none transparent, 1..15 transparent), and the PSNR over the three colour
channels from icamd_measure_error_device.
Method (scripts/bench_etc2_th.py): untimed preconditioning calls, then device events around K back-to-back calls, repeated.
Checks, per leg and mode: every block of image 0 that differs from DEFAULT is a planar (PLANAR_TH: planar, T or H) word, the
summed squared error does not exceed DEFAULT's, and the first four block rows equal the numpy definition
(tests/etc2_a1_th_oracle.py: test infrastructure, the checker only).

  python scripts/bench_etc2_colour_modes.py [--k 5] [--reps 5] [--size 4096] [--images 16] [--strategy 2]
                                            [--codecs 16,21] [--contents noise,smooth,edge,edge_blobs]
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
import etc2_a1_th_oracle as M  # noqa: E402
import etc2_colour_oracle as C  # noqa: E402
import etc2_th_oracle as H  # noqa: E402

MODE_NAMES = ("default", "planar", "planar_th")


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


def image(content, s):
    """(s, s, 4) uint8: the content's colours, alpha 255 (edge_blobs: the tiled cut-out mask)."""
    reps = (s + 63) // 64
    if content in ("edge", "edge_blobs"):
        base = np.tile(H.edges(0)[..., :3].astype(np.int64), (reps, reps, 1))[:s, :s]
        g = np.random.Generator(np.random.PCG64(9740))
        rgb = np.clip(base + g.integers(-6, 7, base.shape), 0, 255)
    else:
        rgb = B.image(content, s, s, 4, index=1).reshape(s, s, 4)[..., :3]
    img = np.full((s, s, 4), 255, np.uint8)
    img[..., :3] = rgb
    if content == "edge_blobs":
        img[..., 3] = np.tile(A.alpha_blobs(64, 64), (reps, reps))[:s, :s]
    return img


def colour_modes_of(codec, words):
    """The mode of every block's colour word (an ETC2 RGBA8 colour word has an individual mode, an ETC2 RGB8A1 word has not)."""
    return C.modes(words[:, -8:]) if codec == M.ETC2_RGBA8 else A.modes(words[:, -8:])


def shares(codec, words, img0, s):
    """Shares of image 0's blocks by the mode of the colour word; ETC2 RGB8A1: also within each block class."""
    m = colour_modes_of(codec, words)
    out = {"planar_share": round(float((m == A.PLANAR).mean()), 4), "t_share": round(float((m == A.T_MODE).mean()), 4),
           "h_share": round(float((m == A.H_MODE).mean()), 4)}
    if codec == M.ETC2_RGB8A1:
        opq = (img0[..., 3] >= 128).reshape(s // 4, 4, s // 4, 4).sum(axis=(1, 3)).reshape(-1)
        for name, sel in (("clear", opq == 0), ("opaque", opq == 16), ("mixed", (opq > 0) & (opq < 16))):
            out[name + "_blocks_share"] = round(float(sel.mean()), 4)
            if sel.any():
                out[name + "_planar_t_h_shares"] = [round(float((m[sel] == k).mean()), 4) for k in (A.PLANAR, A.T_MODE, A.H_MODE)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--strategy", type=int, default=2)
    ap.add_argument("--codecs", default="16,21")
    ap.add_argument("--contents", default="noise,smooth,edge,edge_blobs")
    a = ap.parse_args()
    assert a.size % 4 == 0
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s, n, strategy = a.size, a.images, a.strategy
    strip_rows = min(16, s)
    bad = False
    for codec in [int(c) for c in a.codecs.split(",") if c]:
        per = pkg.encoded_size(codec, s, s)
        bb = per // ((s // 4) * (s // 4))
        outs = [torch.empty((n, per), dtype=torch.uint8, device=dev) for _ in range(3)]
        oracle = M.oracle_encode_rgba8 if codec == M.ETC2_RGBA8 else M.oracle_encode
        for content in [c for c in a.contents.split(",") if c]:
            if content == "edge_blobs" and codec != M.ETC2_RGB8A1:
                continue
            img0 = image(content, s)
            src = torch.from_numpy(img0).to(dev).reshape(1, -1).repeat(n, 1)
            ms, sse, words = [], [], []
            for modes in (0, 1, 2):
                fn = lambda: pkg.encode_etc2_colour_device(codec, src, s, s, 4, etc_strategy=strategy, n_images=n,  # noqa: E731
                                                           out=outs[modes], colour_modes=modes)
                ms.append(time_launches(fn, a.k, a.reps, a.warmup))
                e, _ = pkg.measure_error_device(codec, src, outs[modes].reshape(-1), s, s, 4, n_images=n)
                torch.cuda.synchronize()
                sse.append(int(e[0, :3].sum().item()))
                words.append(outs[modes][0].cpu().numpy().reshape(-1, bb))
            line = {"codec": codec, "content": content, "strategy": strategy, "images": n, "size": s}
            med0 = statistics.median(ms[0])
            ok = True
            for modes in (0, 1, 2):
                name, med = MODE_NAMES[modes], statistics.median(ms[modes])
                line[name + "_ms_per_call_median"] = round(med, 4)
                line[name + "_ms_min"], line[name + "_ms_max"] = round(min(ms[modes]), 4), round(max(ms[modes]), 4)
                line[name + "_psnr_rgb_db"] = psnr(sse[modes], 3 * s * s)
                if modes:
                    line[name + "_ratio_to_default"] = round(med / med0, 3)
                    line[name + "_pass_ms"] = round(med - med0, 4)
                    line[name] = shares(codec, words[modes], img0, s)
                    diff = (words[modes] != words[0]).any(axis=1)
                    m = colour_modes_of(codec, words[modes][diff])
                    allowed = (m == A.PLANAR) if modes == 1 else ((m == A.PLANAR) | (m == A.T_MODE) | (m == A.H_MODE))
                    want = oracle(img0[:strip_rows], strip_rows, s, 0, strategy, modes=modes)
                    ok &= bool(allowed.all()) and sse[modes] <= sse[0] and words[modes][:len(want) // bb].tobytes() == want
                    line[name + "_changed_share"] = round(float(diff.mean()), 4)
            line["check"] = "changed blocks are planar / T / H words, sse <= default, first rows = definition (image 0)" if ok else "MISMATCH"
            bad |= not ok
            print(json.dumps(line), flush=True)
            del src
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
