#!/usr/bin/env python3
"""Device-resident timing of the BC7 / BC6H mip chains (icamd_encode_bc7_mips_device, icamd_encode_bc6h_mips_device) and of the
half-float pixel pyramid (icamd_mip_pyramid_f16_device), include/ic_amd.h; DESIGN.md 3.25.

Per leg (BC7 DEFAULT from RGBA8, BC7 EXTENDED from RGB888, BC6H UF16 DEFAULT and BC6H SF16 EXTENDED from RGBA16F) and per workload
-- 16 x 4096^2, the bulk case, and 64 x 256^2, the batch of small textures where the launch count dominates -- two variants in
the same process on the same inputs:
  chain   the new call: the pyramid passes, then every level of every image in one encode launch
  route   what a caller had to write before: the pixel pyramid (icamd_mip_pyramid_device / icamd_mip_pyramid_f16_device), then
          icamd_encode_bc7_device / icamd_encode_bc6h_modes_device on level 0 and on every level of the pyramid: 1 + L calls
and, for the BC6H legs, the half-float pyramid alone with the share of 8 TB/s its bytes (source read once + pyramid written)
amount to.
Method: untimed warm-up calls of every variant (code objects loaded, clocks and caches in the state the timed calls meet), then
`reps` repetitions in each of which the variants are timed in turn (device events around k back-to-back calls; the turn starts
one variant later in every repetition); the median and min / max of ms per call are reported, and route / chain with the
spread of the route beside it.  "No slower" means: the chain's median within the route's min - max of this run.
Parity: every byte of the first and the last image of the chain against the route; exit status 1 if any differs.

  python scripts/bench_bptc_mips.py [--k 5] [--reps 5] [--warmup 2] [--legs ...] [--loads 4096,256] [--out profiles/bptc_mips_bench.jsonl]
One JSON line per (leg, workload), printed and appended to --out."""
import argparse
import datetime
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
import bc6h_oracle as B6  # noqa: E402
import ic_testlib as T  # noqa: E402

LEGS = {  # name: (codec, channels, modes)
    "bc7_rgba8": (pkg.BC7, 4, pkg.BC7_MODES_DEFAULT), "bc7_modes_rgb888": (pkg.BC7, 3, pkg.BC7_MODES_EXTENDED),
    "bc6h_uf16_rgba16f": (pkg.BC6H_UF16, 4, pkg.BC6H_MODES_DEFAULT), "bc6h_modes_sf16_rgba16f": (pkg.BC6H_SF16, 4, pkg.BC6H_MODES_EXTENDED),
}
LOADS = {"4096": (16, 4096), "256": (64, 256)}  # name: (images, size)
HBM_BYTES_PER_S = 8e12


def timed(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / k


def bench(leg, load, a, dev):
    codec, chans, modes = LEGS[leg]
    n, s = LOADS[load]
    halves = codec != pkg.BC7
    bpp = chans * (2 if halves else 1)
    lib, st = pkg.lib(), pkg._stream_handle()
    levels = pkg.mip_max_levels(s, s)
    if halves:
        img = B6.content("gradient", s, s, chans, seed=1).view(np.uint8).reshape(-1)
    else:
        img = T.s_mixed(s, s, chans, index=1).reshape(-1)
    src = torch.from_numpy(img.copy()).to(dev).repeat(n)
    img_bytes = s * s * bpp
    total, offs = pkg.bptc_mip_chain_size(codec, s, s)
    out = torch.zeros((n, total), dtype=torch.uint8, device=dev)
    out_r = torch.zeros((n, total), dtype=torch.uint8, device=dev)
    ws = torch.empty((max(2, pkg.bptc_mip_workspace_size(codec, chans, s, s, levels, n)),), dtype=torch.uint8, device=dev)
    pyr_per, poffs = pkg.mip_pyramid_size(bpp, s, s, levels)
    pyr = torch.empty((n, max(pyr_per, 2)), dtype=torch.uint8, device=dev)

    def encode_level(h, w, stride, src_ptr, src_image_stride, dst_ptr, dst_image_stride):
        if halves:
            rc = lib.icamd_encode_bc6h_modes_device(codec, modes, chans, h, w, h, w, stride, n, src_image_stride, dst_image_stride, src_ptr,
                                                    dst_ptr, st)
        else:
            rc = lib.icamd_encode_bc7_device(modes, chans, 0, h, w, h, w, stride, n, src_image_stride, dst_image_stride, src_ptr, dst_ptr, st)
        assert rc == 0, rc

    def pyramid():
        if halves:
            rc = lib.icamd_mip_pyramid_f16_device(chans, s, s, s * bpp, levels, n, img_bytes, pyr_per, src.data_ptr(), pyr.data_ptr(), st)
        else:
            rc = lib.icamd_mip_pyramid_device(chans, s, s, s * bpp, levels, n, img_bytes, pyr_per, src.data_ptr(), pyr.data_ptr(), st)
        assert rc == 0, rc

    def chain():
        if halves:
            pkg.encode_bc6h_mips_device(codec, src, s, s, chans, bc6h_modes=modes, n_images=n, out=out, workspace=ws)
        else:
            pkg.encode_bc7_mips_device(src, s, s, chans, bc7_modes=modes, n_images=n, out=out, workspace=ws)

    def route():
        pyramid()
        encode_level(s, s, s * bpp, src.data_ptr(), img_bytes, out_r.data_ptr(), total)
        for l in range(1, levels):
            lh, lw = pkg.mip_level_shape(s, s, l)
            encode_level(lh, lw, lw * bpp, pyr.data_ptr() + poffs[l - 1], pyr_per, out_r.data_ptr() + offs[l], total)

    variants = (("chain", chain), ("route", route)) + ((("pyramid_f16", pyramid),) if halves else ())
    for _, fn in variants:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    k = a.k if s >= 1024 else a.k * 20  # (small textures: enough calls for a window of some tens of milliseconds)
    times = {name: [] for name, _ in variants}
    m = len(variants)
    for r in range(a.reps):
        for name, fn in variants[r % m:] + variants[:r % m]:
            times[name].append(timed(fn, k))
    pyramid_passes = 0 if levels == 1 else 1 if levels <= 7 or s <= 128 else 2
    rec = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "leg": leg, "n_images": n, "size": s,
           "levels": levels, "k": k, "reps": a.reps, "kernel": pkg.bptc_mip_kernel_name(codec, chans, modes),
           "launches_chain": pyramid_passes + 1, "launches_route": pyramid_passes + levels}
    med = {}
    for name, t in times.items():
        med[name] = statistics.median(t)
        rec[name + "_ms"] = round(med[name], 4)
        rec[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
    rec["chain_over_route"] = round(med["chain"] / med["route"], 4)
    rec["route_spread"] = round((max(times["route"]) - min(times["route"])) / med["route"], 4)
    rec["chain_within_route_min_max"] = bool(med["chain"] <= max(times["route"]))
    if halves:
        moved = n * (img_bytes + pyr_per)  # the source read once + the pyramid written
        rec["pyramid_f16_bytes"] = moved
        rec["pyramid_f16_share_of_8TBps"] = round(moved / (med["pyramid_f16"] * 1e-3) / HBM_BYTES_PER_S, 4)
    out.zero_()
    route()
    chain()
    torch.cuda.synchronize()
    same = bool(torch.equal(out[0], out_r[0]) and torch.equal(out[n - 1], out_r[n - 1]))
    rec["parity_chain_vs_route"] = same
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    del src, out, out_r, ws, pyr
    torch.cuda.empty_cache()
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--loads", default=",".join(LOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bptc_mips_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bptc_mips.py needs a GPU: the backend has no CPU path")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ok = True
    for load in a.loads.split(","):
        for leg in a.legs.split(","):
            ok &= bench(leg, load, a, dev)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
