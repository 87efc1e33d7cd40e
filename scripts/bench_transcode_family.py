#!/usr/bin/env python3
"""Device-resident throughput of the in-place DXT1 -> ETC2 RGB8, BC4 -> EAC R11 and BC5 -> EAC RG11 transcodes (extensions,
include/ic_amd.h), each against the route a caller had before it.

Input per transcode: 16 x 4096^2 worth of source blocks made by the library's own encoder from the "mixed" generator (3, 1 and 2
channels of it).  Legs, all in one run on the same blocks, per transcode:
  (a) transcode   the in-place transcode; the input is restored between launches OUTSIDE the timed region, so every launch is
                  timed on its own, between two device events;
  (b) route       icamd_decode_device(source codec) into a pixel image + icamd_encode_device(target codec; kHeuristic for ETC2
                  RGB8) of that image.
The two legs ALTERNATE launch by launch, after untimed preconditioning launches of both; reps x k timed launches per leg; the
median, min and max of ms per launch, and (max - min) / median as the spread.
Parity: (a)'s output equals (b)'s output, every byte of every image; the first four block rows of image 0 also equal the
definition (tests/transcode_family_oracle.py: test infrastructure, the checker only).
For DXT1 also, for information only (no threshold): the share of blocks that became planar, and the PSNR of the ETC2 RGB8 result
and of the DXT1 -> ETC1 result of the same blocks against the DXT1-decoded pixels, through icamd_measure_error_device.
One JSON line per leg, one summary line per transcode.

  python scripts/bench_transcode_family.py [--k 5] [--reps 5] [--size 4096] [--images 16] [--only dxt1,bc4,bc5]
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
import transcode_family_oracle as X  # noqa: E402

# kind -> (source codec, target codec, components, block bytes, device symbol)
KINDS = {"dxt1": (pkg.DXT1, pkg.ETC2_RGB8, 3, 8, "icamd_transcode_dxt1_to_etc2_rgb8_device"),
         "bc4": (pkg.BC4, pkg.EAC_R11, 1, 8, "icamd_transcode_bc4_to_eac_r11_device"),
         "bc5": (pkg.BC5, pkg.EAC_RG11, 2, 16, "icamd_transcode_bc5_to_eac_rg11_device")}


def time_alternating(legs, k, reps, warmup):
    """legs: [(fn, restore)].  ms of each of reps * k launches of every leg, the legs taking turns; restore() runs before its
    leg's launch, outside the events."""
    for _ in range(warmup):
        for fn, restore in legs:
            restore()
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in legs]
    for _ in range(reps * k):
        for i, (fn, restore) in enumerate(legs):
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[i].append(e0.elapsed_time(e1))
    return out


def leg(name, ms, n_blocks, parity, **more):
    m = statistics.median(ms)
    rec = {"leg": name, "launches": len(ms), "ms_per_launch_median": round(m, 4), "ms_min": round(min(ms), 4),
           "ms_max": round(max(ms), 4), "spread": round((max(ms) - min(ms)) / m, 4),
           "gblocks_per_s": round(n_blocks / (m * 1e-3) / 1e9, 3), "parity": bool(parity)}
    rec.update(more)
    print(json.dumps(rec), flush=True)
    return m


def run_kind(kind, a, dev, lib, stream):
    src_codec, dst_codec, comps, block, symbol = KINDS[kind]
    s, n = a.size, a.images
    img0 = B.image(a.content, s, s, comps, index=1)
    src_px = torch.from_numpy(img0).to(dev).reshape(1, -1).repeat(n, 1)
    blocks = pkg.encode_device(src_codec, src_px, s, s, comps, n_images=n)  # [n, bytes]: the input of both legs
    del src_px
    per = blocks.shape[1]
    n_blocks = n * per // block
    work = torch.empty_like(blocks)
    pixels = torch.empty((n, s * s * comps), dtype=torch.uint8, device=dev)
    out_b = torch.empty_like(blocks)
    fn = getattr(lib, symbol)

    def transcode():
        rc = fn(ctypes.c_void_p(work.data_ptr()), work.numel(), stream)
        assert rc == 0, rc

    def route():
        rc = lib.icamd_decode_device(src_codec, 0, s, s, 0, n, per, s * s * comps, ctypes.c_void_p(blocks.data_ptr()),
                                     ctypes.c_void_p(pixels.data_ptr()), stream)
        assert rc == 0, rc
        rc = lib.icamd_encode_device(dst_codec, pkg.ETC_HEURISTIC, comps, 0, s, s, s, s, s * comps, n, s * s * comps, per,
                                     ctypes.c_void_p(pixels.data_ptr()), ctypes.c_void_p(out_b.data_ptr()), stream)
        assert rc == 0, rc

    ms_a, ms_b = time_alternating([(transcode, lambda: work.copy_(blocks)), (route, lambda: None)], a.k, a.reps, a.warmup)
    torch.cuda.synchronize()

    rows = min(4, s // 4) * (s // 4)  # the first four block rows of image 0, against the definition
    head = blocks[0, :rows * block].cpu().numpy().tobytes()
    same = bool(torch.equal(work, out_b))
    defined = work[0, :rows * block].cpu().numpy().tobytes() == X.ORACLE[kind](head)

    more = {}
    if kind == "dxt1":  # the planar share, and what the planar mode buys over the DXT1 -> ETC1 transcode of the same blocks
        etc1 = blocks.clone()
        rc = lib.icamd_transcode_dxt1_to_etc1_device(ctypes.c_void_p(etc1.data_ptr()), etc1.numel(), stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        differs = (work.reshape(-1, 8) != etc1.reshape(-1, 8)).any(dim=1)  # a block is the ETC1 word unless it is planar
        more["planar_share"] = round(float(differs.float().mean().item()), 4)
        for label, codec, result in (("psnr_etc2_rgb8_db", pkg.ETC2_RGB8, work), ("psnr_etc1_db", pkg.ETC1, etc1)):
            sse, _ = pkg.measure_error_device(codec, pixels, result, s, s, 3, n_images=n)
            torch.cuda.synchronize()
            more[label] = round(pkg.psnr_from_stats(sse[0].cpu().numpy()[:3], s * s, 3), 3)
        del etc1

    common = {"images": n, "size": s, "content": a.content, "bytes": n * per}
    m_a = leg("transcode_" + kind, ms_a, n_blocks, same and defined, equals_route=same, equals_definition=defined, **common, **more)
    m_b = leg("route_" + kind, ms_b, n_blocks, same, **common)
    # "faster" only beyond the run-to-run spread of both legs: the slowest transcode launch against the fastest route launch
    print(json.dumps({"summary": kind + ": transcode / route", "ratio": round(m_a / m_b, 3),
                      "transcode_faster_beyond_spread": bool(max(ms_a) < min(ms_b)), "parity": bool(same and defined)}), flush=True)
    return same and defined


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--content", default="mixed", choices=sorted(B.GENERATORS))
    ap.add_argument("--only", default="dxt1,bc4,bc5")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = pkg.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = True
    for kind in a.only.split(","):
        ok = run_kind(kind, a, dev, lib, stream) and ok
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
