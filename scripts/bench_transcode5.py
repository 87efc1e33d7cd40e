#!/usr/bin/env python3
"""Device-resident throughput of the in-place DXT5 -> ETC2 RGBA8 transcode (extension, include/ic_amd.h
icamd_transcode_dxt5_to_etc2_rgba8_device) against the route a caller had before it.

Input: 16 x 4096^2 worth of DXT5 blocks (256 MiB) made by the library's own DXT5 encoder from the "mixed" generator.  Legs, all
in one run on the same blocks:
  (a) transcode   the in-place transcode; the input is restored between launches OUTSIDE the timed region, so every launch is
                  timed on its own, between two device events;
  (b) route       icamd_decode_device(DXT5) into an RGBA8 image + icamd_encode_device(ETC2_RGBA8, kHeuristic) of that image;
  (c) dxt1_etc1   icamd_transcode_dxt1_to_etc1_device on the same number of BYTES (twice the blocks), for scale; restored alike.
Method: untimed preconditioning launches, then reps x k timed launches per leg; the median, min and max of ms per launch.
Parity: (a)'s output equals (b)'s output, every byte of every image; its first four block rows also equal the numpy / C-oracle
definition (tests/transcode5_oracle.py: test infrastructure, the checker only); (c) against the C oracle on the same rows.
Also printed, for information only (no threshold): the PSNR of the transcoded blocks against the DXT5-decoded pixels, through
icamd_measure_error_device.  One JSON line per leg, then a summary line.

  python scripts/bench_transcode5.py [--k 5] [--reps 5] [--size 4096] [--images 16]
Exit status 1 if any parity flag is false."""
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
import ic_testlib as T  # noqa: E402
import transcode5_oracle as X  # noqa: E402


def time_each(fn, restore, k, reps, warmup):
    """ms of each of reps * k launches of fn; restore() runs before every launch, outside the events."""
    for _ in range(warmup):
        restore()
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps * k):
        restore()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def leg(name, ms, n_blocks, parity, **more):
    m = statistics.median(ms)
    rec = {"leg": name, "launches": len(ms), "ms_per_launch_median": round(m, 4), "ms_min": round(min(ms), 4),
           "ms_max": round(max(ms), 4), "gblocks_per_s": round(n_blocks / (m * 1e-3) / 1e9, 3), "parity": bool(parity)}
    rec.update(more)
    print(json.dumps(rec), flush=True)
    return m


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
    lib = pkg.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    img0 = B.image(a.content, s, s, 4, index=1)
    rgba = torch.from_numpy(img0).to(dev).reshape(1, -1).repeat(n, 1)
    dxt5 = pkg.encode_device(pkg.DXT5, rgba, s, s, 4, n_images=n)  # [n, bytes]: the input of every leg
    del rgba
    per = dxt5.shape[1]
    n_blocks = n * per // 16
    work = torch.empty_like(dxt5)
    restore = lambda: work.copy_(dxt5)  # noqa: E731

    # (a) the in-place transcode
    def transcode():
        rc = lib.icamd_transcode_dxt5_to_etc2_rgba8_device(ctypes.c_void_p(work.data_ptr()), work.numel(), stream)
        assert rc == 0, rc
    ms_a = time_each(transcode, restore, a.k, a.reps, a.warmup)
    torch.cuda.synchronize()
    got_a = work.clone()

    # (b) decode to pixels, encode the pixels
    pixels = torch.empty((n, s * s * 4), dtype=torch.uint8, device=dev)
    out_b = torch.empty_like(dxt5)

    def route():
        rc = lib.icamd_decode_device(pkg.DXT5, 0, s, s, 0, n, per, s * s * 4, ctypes.c_void_p(dxt5.data_ptr()),
                                     ctypes.c_void_p(pixels.data_ptr()), stream)
        assert rc == 0, rc
        rc = lib.icamd_encode_device(pkg.ETC2_RGBA8, pkg.ETC_HEURISTIC, 4, 0, s, s, s, s, s * 4, n, s * s * 4, per,
                                     ctypes.c_void_p(pixels.data_ptr()), ctypes.c_void_p(out_b.data_ptr()), stream)
        assert rc == 0, rc
    ms_b = time_each(route, lambda: None, a.k, a.reps, a.warmup)
    torch.cuda.synchronize()

    rows = min(4, s // 4) * (s // 4)  # the first four block rows of image 0, against the definition
    head = dxt5[0, :rows * 16].cpu().numpy().tobytes()
    want_head = X.oracle_transcode5(head)
    same = bool(torch.equal(got_a, out_b))
    defined = got_a[0, :rows * 16].cpu().numpy().tobytes() == want_head

    # PSNR of the result against the pixels the DXT5 blocks decode to (information only)
    sse, mx = pkg.measure_error_device(pkg.ETC2_RGBA8, pixels, got_a, s, s, 4, n_images=n)
    torch.cuda.synchronize()
    sse0, mx0 = sse[0].cpu().numpy(), mx[0].cpu().numpy()
    psnr = {"psnr_rgba_db": round(pkg.psnr_from_stats(sse0, s * s, 4), 2), "psnr_rgb_db": round(pkg.psnr_from_stats(sse0[:3], s * s, 3), 2),
            "psnr_alpha_db": round(pkg.psnr_from_stats(sse0[3:], s * s, 1), 2), "max_abs": [int(v) for v in mx0]}
    del pixels, out_b

    # (c) DXT1 -> ETC1 on the same bytes
    def dxt1():
        rc = lib.icamd_transcode_dxt1_to_etc1_device(ctypes.c_void_p(work.data_ptr()), work.numel(), stream)
        assert rc == 0, rc
    ms_c = time_each(dxt1, restore, a.k, a.reps, a.warmup)
    torch.cuda.synchronize()
    ok_c = work[0, :rows * 16].cpu().numpy().tobytes() == T.oracle_transcode(head)

    common = {"images": n, "size": s, "content": a.content, "bytes": n * per}
    m_a = leg("transcode_dxt5_to_etc2_rgba8", ms_a, n_blocks, same and defined, equals_route=same, equals_definition=defined,
              **common, **psnr)
    m_b = leg("decode_dxt5_then_encode_etc2_rgba8_heuristic", ms_b, n_blocks, same, **common)
    m_c = leg("transcode_dxt1_to_etc1_same_bytes", ms_c, 2 * n_blocks, ok_c, **common)
    print(json.dumps({"summary": "transcode / route", "ratio": round(m_a / m_b, 3), "transcode_faster": bool(m_a < m_b),
                      "transcode_over_dxt1_to_etc1": round(m_a / m_c, 2), "parity": bool(same and defined and ok_c)}), flush=True)
    return 0 if (same and defined and ok_c) else 1


if __name__ == "__main__":
    sys.exit(main())
