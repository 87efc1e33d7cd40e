#!/usr/bin/env python3
"""Device-resident throughput and quality of the BC1A (BC1 with punch-through alpha) and BC2 encoders, decoders and metrics
(extensions, include/ic_amd.h ICAMD_BC1A / ICAMD_BC2) next to the kernels they are built on, in the same run: BC1A
beside ICAMD_DXT1 from RGBA8 and ICAMD_ETC2_RGB8A1, BC2 beside ICAMD_DXT5.

Contents, 16 x 4096^2 RGBA8: "opaque_noise" and "opaque_smooth" (alpha 255: BC1A runs the DXT1 colour block alone and moves the
bytes ICAMD_DXT1 moves, BC2 the bytes ICAMD_DXT5 moves), "cutout" (the smooth colour under the blobby alpha mask of
scripts/bench_etc2_a1.py, a 256 x 256 tile repeated) and "cutout_noise_alpha" (the same colour, alpha uniform noise: nearly every
block takes the masked path).
Reported per content: the median ms per launch of every leg with its run-to-run spread (min / max over the repetitions), the
ratios BC1A / DXT1, BC1A / ETC2 RGB8A1 and BC2 / DXT5, the encoders' algorithmic bytes (source + blocks) over the median time as a
fraction of 8 TB/s, decode and metric ms of both codecs, the share of blocks of image 0 that are all-transparent, mixed or opaque,
and the four-channel PSNR of BC1A, BC2, DXT5 and ETC2 RGB8A1 from icamd_measure_error_device.
Method: untimed preconditioning calls of every leg, then device events around K back-to-back launches, repeated, the legs
alternating within every repetition.
Checks, per content: the first four block rows of image 0 of both codecs equal the numpy statement (tests/bc1a_bc2_oracle.py:
test infrastructure, the checker only); on the opaque contents the BC1A stream equals the DXT1 stream; BC2's colour halves equal
DXT5's.

  python scripts/bench_bc1a_bc2.py [--k 5] [--reps 5] [--size 4096] [--images 16]
                                   [--contents opaque_noise,opaque_smooth,cutout,cutout_noise_alpha] > profiles/bc1a_bc2_bench.jsonl
Exit status 1 if any check fails."""
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
import bc1a_bc2_oracle as O  # noqa: E402
import bc45_oracle as B  # noqa: E402
import etc2_a1_oracle as A  # noqa: E402

PEAK_BYTES_PER_S = 8e12  # HBM3E of one MI355X


def time_launches(fns, k, reps, warmup):
    """{name: fn} -> {name: [ms per launch, one per repetition]}; the legs alternate within every repetition, so that a drift of
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
    img = B.image("noise" if content == "opaque_noise" else "smooth", s, s, 4, index=1).copy()
    if content.startswith("cutout"):
        if content == "cutout":
            tile = A.alpha_blobs(min(s, 256), min(s, 256), index=1)
        else:
            tile = np.random.Generator(np.random.PCG64(36)).integers(0, 256, (min(s, 256), min(s, 256)), dtype=np.uint8)
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
    ap.add_argument("--contents", default="opaque_noise,opaque_smooth,cutout,cutout_noise_alpha")
    a = ap.parse_args()
    if a.size % 4:
        ap.error("--size must be a multiple of 4")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s, n = a.size, a.images
    per8, per16 = O.encoded_size(O.BC1A, s, s), O.encoded_size(O.BC2, s, s)
    outs = {name: torch.empty((n, per), dtype=torch.uint8, device=dev)
            for name, per in (("bc1a", per8), ("dxt1", per8), ("etc2_a1", per8), ("bc2", per16), ("dxt5", per16))}
    codecs = {"bc1a": pkg.BC1A, "dxt1": pkg.DXT1, "etc2_a1": pkg.ETC2_RGB8A1, "bc2": pkg.BC2, "dxt5": pkg.DXT5}
    stats = torch.empty((n, pkg.ERROR_STATS_BYTES), dtype=torch.uint8, device=dev)
    decoded = torch.empty((n, s * s * 4), dtype=torch.uint8, device=dev)
    strip_rows = min(16, s)
    bad = False
    for content in [c for c in a.contents.split(",") if c]:
        img0 = content_image(content, s)
        src = torch.from_numpy(img0).to(dev).reshape(1, -1).repeat(n, 1)
        n_opq = (img0[..., 3] >= 128).reshape(s // 4, 4, s // 4, 4).sum(axis=(1, 3)).reshape(-1)
        shares = {"all_transparent": float((n_opq == 0).mean()), "mixed": float(((n_opq > 0) & (n_opq < 16)).mean()),
                  "opaque": float((n_opq == 16).mean())}

        def enc(name):
            return lambda: pkg.encode_device(codecs[name], src, s, s, 4, n_images=n, out=outs[name])

        ms = time_launches({name: enc(name) for name in codecs}, a.k, a.reps, a.warmup)
        torch.cuda.synchronize()
        # decode and metric of the two new codecs on the encoders' output, into caller-owned buffers (the C ABI's decoder: the
        # Python wrapper would allocate and clear its RGBA8 rows inside the timed window)
        more = {}
        for name in ("bc1a", "bc2"):
            blocks = outs[name].reshape(-1)
            more["decode_" + name] = lambda c=codecs[name], b=blocks: pkg.lib().icamd_decode_device(
                c, 0, s, s, 0, n, b.numel() // n, s * s * 4, b.data_ptr(), decoded.data_ptr(), None)
            more["metric_" + name] = lambda c=codecs[name], b=blocks: pkg.measure_error_device(c, src, b, s, s, 4, n_images=n, out=stats)
        ms.update(time_launches(more, a.k, a.reps, a.warmup))
        sse = {}
        for name in ("bc1a", "bc2", "dxt5", "etc2_a1"):
            sse[name] = pkg.measure_error_device(codecs[name], src, outs[name].reshape(-1), s, s, 4, n_images=n)[0][0].cpu().numpy()
        torch.cuda.synchronize()
        host = {name: outs[name][0].cpu().numpy() for name in outs}
        ok = True
        for codec, name in ((O.BC1A, "bc1a"), (O.BC2, "bc2")):
            want = O.oracle_encode(codec, img0[:strip_rows], strip_rows, s)
            ok &= host[name][:len(want)].tobytes() == want
        if content.startswith("opaque"):
            ok &= host["bc1a"].tobytes() == host["dxt1"].tobytes()
        ok &= bool((host["bc2"].reshape(-1, 16)[:, 8:] == host["dxt5"].reshape(-1, 16)[:, 8:]).all())
        bad |= not ok
        med = {name: statistics.median(v) for name, v in ms.items()}
        pixels = n * s * s
        print(json.dumps({
            "content": content, "images": n, "size": s,
            "ms": {name: spread(v) for name, v in ms.items()},
            "ratio_bc1a_over_dxt1": round(med["bc1a"] / med["dxt1"], 3),
            "ratio_bc1a_over_etc2_a1": round(med["bc1a"] / med["etc2_a1"], 3),
            "ratio_bc2_over_dxt5": round(med["bc2"] / med["dxt5"], 3),
            # algorithmic bytes: 4 per pixel read, 0.5 (8-byte blocks) or 1 (16-byte blocks) per pixel written
            "fraction_of_8_tb_per_s": {name: round(pixels * (4.5 if name in ("bc1a", "dxt1") else 5.0) / (med[name] * 1e-3) / PEAK_BYTES_PER_S, 3)
                                       for name in ("bc1a", "dxt1", "bc2", "dxt5")},
            "class_shares": {k: round(v, 4) for k, v in shares.items()},
            "psnr_rgba_db": {name: psnr(int(v.sum()), 4 * s * s) for name, v in sse.items()},
            "check": "first rows = statement, opaque BC1A = DXT1, BC2 colour = DXT5 colour (image 0)" if ok else "MISMATCH"}), flush=True)
        del src
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
