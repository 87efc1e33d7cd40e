#!/usr/bin/env python3
"""Device-resident timing of the ETC2-family mip chains (icamd_encode_etc2_mips_device, include/ic_amd.h).

Per codec (ETC2 RGB8, RGB8 with T / H, RGBA8, RGB8A1, EAC R11, EAC RG11; RGBA8 sources throughout, kSmallerError) and per workload
-- 16 x 4096^2, the bulk case, and 64 x 256^2, the batch of small textures where the launch count dominates -- four variants:
  (a)  chain          the new call, levels in its default order inside the launch (largest first)
  (a1) chain_smallest the new call with the smallest level first (icamd_etc2_mip_tune(0)): the other order of DESIGN 3.18
  (b)  level0        level 0 alone through icamd_encode_device / icamd_encode_etc2_device
  (c)  composition   what a caller had to write before: icamd_mip_pyramid_device, then icamd_encode_device (T / H:
                     icamd_encode_etc2_device) on level 0 and on every level of the pyramid -- 1 + L calls, 1 + 2 L launches with T / H
Method: untimed warm-up calls of all four, then `reps` repetitions in each of which the four are timed in turn (device events
around k back-to-back calls; the turn starts one variant later in every repetition), so drift of the clocks and the state the
previous variant leaves hit all alike; the median and min / max of ms per call are reported, and
c / a with the spread of (c) beside it.  The claim to confirm or refute: (a) is not slower than (c) beyond (c)'s own spread at
16 x 4096^2, and faster at 64 x 256^2.
Parity: every byte of the first and the last image of (a), and of (a1), against (c); exit status 1 if any differs.

  python scripts/bench_etc2_mips.py [--k 5] [--reps 8] [--warmup 2] [--legs rgb8,rgb8_th,rgba8,rgb8a1,r11,rg11] [--loads 4096,256]
One JSON line per (leg, workload)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import ic_amd_loader  # noqa: E402

pkg = ic_amd_loader.load_package()
import ic_testlib as T  # noqa: E402

LEGS = {  # name: (codec, etc2_modes)
    "rgb8": (pkg.ETC2_RGB8, 0), "rgb8_th": (pkg.ETC2_RGB8, pkg.ETC2_MODES_TH), "rgba8": (pkg.ETC2_RGBA8, 0),
    "rgb8a1": (pkg.ETC2_RGB8A1, 0), "r11": (pkg.EAC_R11, 0), "rg11": (pkg.EAC_RG11, 0),
}
LOADS = {"4096": (16, 4096), "256": (64, 256)}  # name: (images, size)
COMPS, STRATEGY = 4, 2


def timed(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / k


def bench(leg, load, a, dev):
    codec, modes = LEGS[leg]
    n, s = LOADS[load]
    lib, st = pkg.lib(), pkg._stream_handle()
    levels = pkg.mip_max_levels(s, s)
    img = T.s_mixed(s, s, COMPS, index=1).reshape(-1)
    src = torch.from_numpy(img.copy()).to(dev).repeat(n)
    img_bytes = s * s * COMPS
    total, offs = pkg.etc2_mip_chain_size(codec, s, s)
    out = torch.zeros((n, total), dtype=torch.uint8, device=dev)
    out_c = torch.zeros((n, total), dtype=torch.uint8, device=dev)
    out_0 = torch.zeros((n, offs[1]), dtype=torch.uint8, device=dev)
    ws = torch.empty((max(1, pkg.etc2_mip_workspace_size(codec, COMPS, s, s, levels, n)),), dtype=torch.uint8, device=dev)
    pyr_per, poffs = pkg.mip_pyramid_size(COMPS, s, s, levels)
    pyr = torch.empty((n, max(pyr_per, 1)), dtype=torch.uint8, device=dev)

    def encode_level(h, w, stride, src_ptr, src_image_stride, dst_ptr, dst_image_stride):
        if modes:
            rc = lib.icamd_encode_etc2_device(codec, STRATEGY, modes, COMPS, 0, h, w, h, w, stride, n, src_image_stride, dst_image_stride,
                                              src_ptr, dst_ptr, st)
        else:
            rc = lib.icamd_encode_device(codec, STRATEGY, COMPS, 0, h, w, h, w, stride, n, src_image_stride, dst_image_stride, src_ptr,
                                         dst_ptr, st)
        assert rc == 0, rc

    def chain():
        pkg.encode_etc2_mips_device(codec, src, s, s, COMPS, etc_strategy=STRATEGY, etc2_modes=modes, n_images=n, out=out, workspace=ws)

    def chain_smallest():
        pkg.etc2_mip_tune(0)
        try:
            chain()
        finally:
            pkg.etc2_mip_tune(1)

    def level0():
        encode_level(s, s, s * COMPS, src.data_ptr(), img_bytes, out_0.data_ptr(), offs[1])

    def composition():
        assert lib.icamd_mip_pyramid_device(COMPS, s, s, s * COMPS, levels, n, img_bytes, pyr_per, src.data_ptr(), pyr.data_ptr(), st) == 0
        encode_level(s, s, s * COMPS, src.data_ptr(), img_bytes, out_c.data_ptr(), total)
        for l in range(1, levels):
            lh, lw = pkg.mip_level_shape(s, s, l)
            encode_level(lh, lw, lw * COMPS, pyr.data_ptr() + poffs[l - 1], pyr_per, out_c.data_ptr() + offs[l], total)

    variants = (("chain", chain), ("chain_smallest", chain_smallest), ("level0", level0), ("composition", composition))
    for _, fn in variants:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    k = a.k if s >= 1024 else a.k * 20  # (small textures: enough calls for a window of some tens of milliseconds)
    times = {name: [] for name, _ in variants}
    for r in range(a.reps):  # (rotated: each variant is timed after each other one in turn -- what ran just before shifts a 256^2 leg by 1 - 2 %)
        for name, fn in variants[r % 4:] + variants[:r % 4]:
            times[name].append(timed(fn, k))
    pyramid_passes = 0 if levels == 1 else 1 if levels <= 7 or s <= 128 else 2
    rec = {"leg": leg, "n_images": n, "size": s, "levels": levels, "k": k, "reps": a.reps,
           "kernel": pkg.etc2_mip_kernel_name(codec, COMPS, STRATEGY, 0),
           "launches_chain": pyramid_passes + (2 if modes else 1), "launches_composition": pyramid_passes + levels * (2 if modes else 1)}
    med = {}
    for name, t in times.items():
        med[name] = statistics.median(t)
        rec[name + "_ms"] = round(med[name], 4)
        rec[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
    rec["composition_over_chain"] = round(med["composition"] / med["chain"], 4)
    rec["composition_spread"] = round((max(times["composition"]) - min(times["composition"])) / med["composition"], 4)
    rec["chain_smallest_over_chain"] = round(med["chain_smallest"] / med["chain"], 4)
    rec["chain_over_level0"] = round(med["chain"] / med["level0"], 4)
    ok = True
    composition()
    for name, fn in variants[:2]:
        out.zero_()
        fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(out[0], out_c[0]) and torch.equal(out[n - 1], out_c[n - 1]))
        rec["parity_%s_vs_composition" % name] = same
        ok &= same
    print(json.dumps(rec), flush=True)
    del src, out, out_c, out_0, ws, pyr
    torch.cuda.empty_cache()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--loads", default=",".join(LOADS))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_etc2_mips.py needs a GPU: the backend has no CPU path")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ok = True
    for load in a.loads.split(","):
        for leg in a.legs.split(","):
            ok &= bench(leg, load, a, dev)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
