#!/usr/bin/env python3
"""Device-resident throughput of the fused mip-chain encode (icamd_encode_mips_device, include/ic_amd.h mip-chain section).

Legs: every codec at 16 x 4096^2 RGBA8 (BC4 / BC5 read bytes 0 / 0-1 of the same source), ETC1 at 64 x 1024^2 RGBA8, DXT1 at
1 x 16384^2 RGBA8.  Three variants per leg:
  (a) fused   the whole chain through icamd_encode_mips_device
  (b) level0  level 0 alone through icamd_encode_device
  (c) unfused level 0 through icamd_encode_device, then icamd_mip_pyramid_device and icamd_encode_device per level
Method as scripts/bench_bc45.py: untimed warm-up calls, device events around K back-to-back calls, repeated; the median and
min / max of ms per call.  Algorithmic bytes = source read once + every level's blocks written once, against 8 TB/s.
Parity: image 0 of (a) against (c) (every level), which the GPU tier pins to the oracle.  PSNR of (a)'s levels against the
pixel pyramid, and of the compressed-domain chain (icamd_downsample_device per level, DXT1 / DXT5 / ETC1), reported only; both
come from the device metric (icamd_measure_error_device: no decoded image, no host reduction).

--filter F (1 = sRGB, 2 = alpha-weighted, 3 = both; include/ic_amd.h "mip filters") times the filtered chain instead: legs dxt1,
dxt5, etc1 and `pyramid` (icamd_mip_pyramid_filtered_device alone), with per leg
  (a)  fused     the filtered chain through icamd_encode_mips_filtered_device (pyramid leg: the filtered pyramid)
  (a0) box       the same call with the box filter, in the same session
  (c)  unfused   level 0 through icamd_encode_device, the filtered pyramid, then icamd_encode_device per level (not for `pyramid`)
and the ratios a / a0 and c / a.  Parity: image 0 of (a) against (c).

--filter 4 (the normal-map filter, BC5 only) times the BC5 chain of a 16 x 4096^2 normal map from RG8 and from RGBA8 sources:
the filtered call against the box call of the same build, after a warm-up of both, in interleaved repeats (normal, box, normal,
box, ...).  Parity: image 0 of the RG8 chain against level 0 through icamd_encode_device + the filtered RG8 pyramid +
icamd_encode_device per level, and the RGBA8 chain against the RG8 chain (BC5 reads R and G only).

  python scripts/bench_mips.py [--k 10] [--reps 5] [--legs dxt1,dxt5,etc1,bc4,bc5,etc1_1024,dxt1_16384] [--no-psnr] [--filter F]
One JSON line per leg; exit status 1 if any parity check fails."""
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
import ic_testlib as T  # noqa: E402

PEAK_BPS = 8e12
LEGS = {  # name: (codec, n_images, size)
    "dxt1": (pkg.DXT1, 16, 4096), "dxt5": (pkg.DXT5, 16, 4096), "etc1": (pkg.ETC1, 16, 4096), "bc4": (pkg.BC4, 16, 4096),
    "bc5": (pkg.BC5, 16, 4096), "etc1_1024": (pkg.ETC1, 64, 1024), "dxt1_16384": (pkg.DXT1, 1, 16384),
}


def time_calls(fn, k, reps, warmup):
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


def psnr(codec, pixels, blocks, lh, lw, ch):
    """PSNR over the first `ch` channels of an lh x lw level: RGBA8 `pixels` against `blocks` (device tensors), 99 if equal."""
    sse, _ = pkg.measure_error_device(codec, pixels, blocks, lh, lw, 4)
    total = int(sse[0, :ch].sum().item())
    return 99.0 if total == 0 else 10 * math.log10(255.0 ** 2 * lh * lw * ch / total)


def bench_filtered(a, dev):
    """--filter: (a) / (a0) / (c) per leg, one JSON line each; True if every parity check held."""
    lib = pkg.lib()
    ok = True
    legs = a.legs.split(",") if a.legs != ",".join(LEGS) else ["dxt1", "dxt5", "pyramid"]
    for leg in legs:
        codec, n, s = (None, 16, 4096) if leg == "pyramid" else LEGS[leg]
        comps, f = 4, a.filter
        levels = pkg.mip_max_levels(s, s)
        img0 = T.s_mixed(s, s, comps, index=1).reshape(s, s, comps).copy()
        rng = np.random.default_rng(1)
        alpha = rng.integers(0, 256, (s, s), dtype=np.uint8)  # runs of 0, runs of 255 and noise: every branch of the weighting
        band = (np.arange(s)[:, None] // 8 + np.arange(s)[None, :] // 8) % 3
        alpha[band == 0] = 0
        alpha[band == 1] = 255
        img0[..., 3] = alpha
        src = torch.from_numpy(img0.reshape(-1).copy()).to(dev).repeat(n)
        pyr_per, poffs = pkg.mip_pyramid_size(comps, s, s, levels)
        pyr = torch.empty((n, pyr_per), dtype=torch.uint8, device=dev)
        st = pkg._stream_handle()
        img_bytes = s * s * comps
        rec = {"leg": leg, "filter": f, "n_images": n, "size": s, "levels": levels, "lib": pkg.LIB_PATH}
        if codec is None:
            variants = (("fused", lambda: pkg.mip_pyramid_device(src, s, s, comps, n_images=n, out=pyr, mip_filter=f)),
                        ("box", lambda: pkg.mip_pyramid_device(src, s, s, comps, n_images=n, out=pyr)))
            rec["kernel"] = pkg.mip_kernel_name(pkg.MIP_PYRAMID, comps, f)
        else:
            total, offs = pkg.mip_chain_size(codec, s, s)
            out = torch.empty((n, total), dtype=torch.uint8, device=dev)
            out_c = torch.empty((n, total), dtype=torch.uint8, device=dev)
            ws = torch.empty((max(1, pkg.mip_workspace_size(codec, comps, s, s, levels, n)),), dtype=torch.uint8, device=dev)

            def unfused():
                lib.icamd_encode_device(codec, 2, comps, 0, s, s, s, s, s * comps, n, img_bytes, total, src.data_ptr(),
                                        out_c.data_ptr(), st)
                lib.icamd_mip_pyramid_filtered_device(comps, f, s, s, s * comps, levels, n, img_bytes, pyr_per, src.data_ptr(),
                                                      pyr.data_ptr(), st)
                for l in range(1, levels):
                    lh, lw = pkg.mip_level_shape(s, s, l)
                    lib.icamd_encode_device(codec, 2, comps, 0, lh, lw, lh, lw, lw * comps, n, pyr_per, total,
                                            pyr.data_ptr() + poffs[l - 1], out_c.data_ptr() + offs[l], st)

            variants = (("fused", lambda: pkg.encode_mips_device(codec, src, s, s, comps, n_images=n, out=out, workspace=ws, mip_filter=f)),
                        ("box", lambda: pkg.encode_mips_device(codec, src, s, s, comps, n_images=n, out=out, workspace=ws)),
                        ("unfused", unfused))
            rec["kernel"] = pkg.mip_kernel_name(codec, comps, f)
        res = {}
        for name, fn in variants:
            t = time_calls(fn, a.k, a.reps, a.warmup)
            res[name] = statistics.median(t)
            rec[name + "_ms"] = round(res[name], 4)
            rec[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
        rec["fused_over_box"] = round(res["fused"] / res["box"], 3)
        if codec is not None:
            variants[0][1]()
            unfused()
            torch.cuda.synchronize()
            rec["parity_fused_vs_unfused"] = bool(torch.equal(out[0], out_c[0]))
            ok &= rec["parity_fused_vs_unfused"]
            rec["unfused_over_fused"] = round(res["unfused"] / res["fused"], 3)
        print(json.dumps(rec), flush=True)
        del src, pyr
        torch.cuda.empty_cache()
    return ok


def bench_normal(a, dev):
    """--filter 4: BC5 from RG8 and RGBA8, normal against box interleaved; one JSON line per source layout."""
    lib = pkg.lib()
    codec, n, s, f = pkg.BC5, 16, 4096, pkg.MIP_FILTER_NORMAL
    levels = pkg.mip_max_levels(s, s)
    total, offs = pkg.mip_chain_size(codec, s, s)
    rng = np.random.default_rng(1)
    ang, tilt = rng.uniform(0, 2 * np.pi, (s, s)), rng.uniform(0, 1, (s, s))  # unit normals, z > 0, one code of noise
    img = rng.integers(0, 256, (s, s, 4), dtype=np.uint8)
    img[..., 0] = np.clip(np.rint(127.5 + 127.5 * tilt * np.cos(ang)) + rng.integers(-1, 2, (s, s)), 0, 255)
    img[..., 1] = np.clip(np.rint(127.5 + 127.5 * tilt * np.sin(ang)) + rng.integers(-1, 2, (s, s)), 0, 255)
    st = pkg._stream_handle()
    chains = {}
    ok = True
    for comps in (2, 4):
        src = torch.from_numpy(np.ascontiguousarray(img[..., :comps]).reshape(-1)).to(dev).repeat(n)
        out = torch.empty((n, total), dtype=torch.uint8, device=dev)
        ws = torch.empty((max(1, pkg.mip_workspace_size(codec, comps, s, s, levels, n)),), dtype=torch.uint8, device=dev)
        fns = {"normal": lambda: pkg.encode_mips_device(codec, src, s, s, comps, n_images=n, out=out, workspace=ws, mip_filter=f),
               "box": lambda: pkg.encode_mips_device(codec, src, s, s, comps, n_images=n, out=out, workspace=ws)}
        for fn in fns.values():  # precondition: both code objects loaded, clocks and caches in their steady state
            time_calls(fn, a.k, 1, a.warmup)
        times = {"normal": [], "box": []}
        for _ in range(a.reps):
            for name in ("normal", "box"):
                times[name] += time_calls(fns[name], a.k, 1, 0)
        rec = {"leg": "bc5_rg8" if comps == 2 else "bc5_rgba8", "filter": f, "n_images": n, "size": s, "levels": levels,
               "kernel": pkg.mip_kernel_name(codec, comps, f), "box_kernel": pkg.mip_kernel_name(codec, comps, 0), "lib": pkg.LIB_PATH}
        for name, t in times.items():
            rec[name + "_ms"] = round(statistics.median(t), 4)
            rec[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
        rec["normal_over_box"] = round(statistics.median(times["normal"]) / statistics.median(times["box"]), 3)
        fns["normal"]()
        torch.cuda.synchronize()
        chains[comps] = out[0].clone()
        if comps == 2:
            pyr_per, poffs = pkg.mip_pyramid_size(2, s, s, levels)
            pyr = torch.empty((1, pyr_per), dtype=torch.uint8, device=dev)
            out_c = torch.empty((total,), dtype=torch.uint8, device=dev)
            lib.icamd_encode_device(codec, 2, 2, 0, s, s, s, s, s * 2, 1, 0, 0, src.data_ptr(), out_c.data_ptr(), st)
            lib.icamd_mip_pyramid_filtered_device(2, f, s, s, s * 2, levels, 1, 0, 0, src.data_ptr(), pyr.data_ptr(), st)
            for l in range(1, levels):
                lh, lw = pkg.mip_level_shape(s, s, l)
                lib.icamd_encode_device(codec, 2, 2, 0, lh, lw, lh, lw, lw * 2, 1, 0, 0, pyr.data_ptr() + poffs[l - 1],
                                        out_c.data_ptr() + offs[l], st)
            torch.cuda.synchronize()
            rec["parity_fused_vs_unfused"] = bool(torch.equal(chains[2], out_c))
            ok &= rec["parity_fused_vs_unfused"]
            del pyr, out_c
        else:
            rec["parity_rgba8_vs_rg8"] = bool(torch.equal(chains[4], chains[2]))
            ok &= rec["parity_rgba8_vs_rg8"]
        print(json.dumps(rec), flush=True)
        del src, out, ws
        torch.cuda.empty_cache()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--no-psnr", action="store_true")
    ap.add_argument("--filter", type=int, default=0, choices=[0, 1, 2, 3, 4])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if a.filter == pkg.MIP_FILTER_NORMAL:
        return 0 if bench_normal(a, dev) else 1
    if a.filter:
        return 0 if bench_filtered(a, dev) else 1
    lib = pkg.lib()
    bad = False
    for leg in a.legs.split(","):
        codec, n, s = LEGS[leg]
        comps = 4
        levels = pkg.mip_max_levels(s, s)
        total, offs = pkg.mip_chain_size(codec, s, s)
        img0 = T.s_mixed(s, s, comps, index=1).reshape(s, s, comps)
        src = torch.from_numpy(img0.reshape(-1).copy()).to(dev)
        src = src.repeat(n) if n > 1 else src
        out = torch.empty((n, total), dtype=torch.uint8, device=dev)
        ws = torch.empty((max(1, pkg.mip_workspace_size(codec, comps, s, s, levels, n)),), dtype=torch.uint8, device=dev)
        pyr_per, poffs = pkg.mip_pyramid_size(comps, s, s, levels)
        pyr = torch.empty((n, pyr_per), dtype=torch.uint8, device=dev)
        out_c = torch.empty((n, total), dtype=torch.uint8, device=dev)
        st = pkg._stream_handle()
        img_bytes = s * s * comps

        def fused():
            pkg.encode_mips_device(codec, src, s, s, comps, n_images=n, out=out, workspace=ws)

        def level0():
            lib.icamd_encode_device(codec, 2, comps, 0, s, s, s, s, s * comps, n, img_bytes, total, src.data_ptr(),
                                    out_c.data_ptr(), st)

        def unfused():
            level0()
            lib.icamd_mip_pyramid_device(comps, s, s, s * comps, levels, n, img_bytes, pyr_per, src.data_ptr(), pyr.data_ptr(), st)
            for l in range(1, levels):
                lh, lw = pkg.mip_level_shape(s, s, l)
                lib.icamd_encode_device(codec, 2, comps, 0, lh, lw, lh, lw, lw * comps, n, pyr_per, total,
                                        pyr.data_ptr() + poffs[l - 1], out_c.data_ptr() + offs[l], st)

        res = {}
        for name, fn in (("fused", fused), ("level0", level0), ("unfused", unfused)):
            t = time_calls(fn, a.k, a.reps, a.warmup)
            res[name] = (statistics.median(t), min(t), max(t))
        unfused()
        torch.cuda.synchronize()
        parity = bool(torch.equal(out[0], out_c[0]))
        bad |= not parity
        written = n * total
        read = n * img_bytes
        rec = {"leg": leg, "codec": codec, "n_images": n, "size": s, "levels": levels, "parity_fused_vs_unfused": parity}
        for name, (med, lo, hi) in res.items():
            rec[name + "_ms"] = round(med, 4)
            rec[name + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
            rec[name + "_mpix_s"] = round(n * s * s / (med * 1e-3) / 1e6, 1)
        rec["fused_alg_GBps"] = round((read + written) / (res["fused"][0] * 1e-3) / 1e9, 1)
        rec["fused_frac_8TBps"] = round((read + written) / (res["fused"][0] * 1e-3) / PEAK_BPS, 3)
        rec["fused_over_level0"] = round(res["fused"][0] / res["level0"][0], 3)
        rec["unfused_over_fused"] = round(res["unfused"][0] / res["fused"][0], 3)
        if not a.no_psnr:
            pyramid = [src[:img_bytes]] + [pyr[0, poffs[l - 1]:poffs[l]] for l in range(1, levels)]  # image 0, RGBA8 levels
            ch = 1 if codec == pkg.BC4 else 2 if codec == pkg.BC5 else 4 if codec == pkg.DXT5 else 3
            rec["psnr_fused"] = []
            for l in range(levels):
                lh, lw = pkg.mip_level_shape(s, s, l)
                rec["psnr_fused"].append(round(psnr(codec, pyramid[l], out[0, offs[l]:offs[l + 1]], lh, lw, ch), 2))
            if codec in (pkg.DXT1, pkg.DXT5, pkg.ETC1):
                comp, fmt = (pkg.COMPRESSOR_ETC, pkg.RGB) if codec == pkg.ETC1 else (pkg.COMPRESSOR_DXTC, pkg.RGB if codec == pkg.DXT1 else pkg.RGBA)
                c3 = 4 if codec == pkg.DXT5 else 3
                base = torch.from_numpy(np.ascontiguousarray(img0[..., :c3]).reshape(-1)).to(dev)
                cur = pkg.encode_device(codec, base, s, s, c3)
                rec["psnr_compressed_domain"] = []
                for l in range(levels):
                    lh, lw = pkg.mip_level_shape(s, s, l)
                    if l:
                        cur = pkg.downsample_device(comp, fmt, cur.view(1, -1), *pkg.mip_level_shape(s, s, l - 1))
                        if cur is None:
                            break
                    rec["psnr_compressed_domain"].append(round(psnr(codec, pyramid[l], cur.reshape(-1).contiguous(), lh, lw, ch), 2))
        print(json.dumps(rec), flush=True)
        del src, out, ws, pyr, out_c
        torch.cuda.empty_cache()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
