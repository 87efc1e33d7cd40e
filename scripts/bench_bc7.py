#!/usr/bin/env python3
"""Device-resident throughput and quality of BC7 (extension, include/ic_amd.h ICAMD_BC7) next to DXT5 in the
same run.

Per content (noise: uniform RGBA noise; smooth: triangle waves with 3 bits of noise; ramp: linear ramps in all four
channels) at 16 x 4096^2 RGBA8:
  bc7 encode, dxt5 encode   icamd_encode_device; ms per launch (median, min, max), the RGBA PSNR of image 0 from
                            icamd_measure_error_device, algorithmic bytes (source read + blocks written, once each) per second
                            and their fraction of 8 TB/s;
  bc7 decode, bc7 metric    icamd_decode_device / icamd_measure_error_device on the encoder's blocks, timed the same way.
One line per content compares the medians and the PSNRs; one line reports the VALU instructions per block of the BC7 kernels
from the compiler's ISA (hipcc -S of csrc/bc7_kernels.hip; skipped without hipcc).  Parity: the first block row of image 0
against the numpy definition (tests/bc7_oracle.py: test infrastructure, the checker only).
Method (scripts/bench_eac11_16.py): untimed preconditioning calls, then device events around K back-to-back launches, repeated.

  python scripts/bench_bc7.py [--k 5] [--reps 5] [--size 4096] [--images 16] [--skip-isa]
Exit status 1 if any leg's parity fails."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ic_amd_loader  # noqa: E402

pkg = ic_amd_loader.load_package()
import bc7_oracle as B  # noqa: E402

HBM_BYTES_PER_S = 8e12


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


def valu_per_block():
    """{kernel: VALU instructions in its ISA} -- static counts, one block per lane, both passes of the search included."""
    if not shutil.which("hipcc"):
        return None
    csrc = os.path.join(ROOT, "image-compression_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "bc7_kernels.s")
        subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                               "-S", "--cuda-device-only", "-o", out, os.path.join(csrc, "bc7_kernels.hip")], stderr=subprocess.DEVNULL)
        text = open(out).read()
    counts = {}
    for name in ("icamd_bc7_rgba8_kernel", "icamd_bc7_rgb888_kernel", "icamd_bc7_decode_kernel"):
        body = text[text.index("\n%s:" % name):]
        body = body[:body.index("s_endpgm")]
        counts[name] = len(re.findall(r"^\s+v_\w+", body, re.M))
    return counts


def line(leg, name, n, s, ms, nbytes, **extra):
    m = statistics.median(ms)
    rate = nbytes / (m * 1e-3)
    rec = {"leg": leg, "content": name, "images": n, "size": s, "ms_per_launch_median": round(m, 4), "ms_min": round(min(ms), 4),
           "ms_max": round(max(ms), 4), "gpixels_per_s": round(n * s * s / (m * 1e-3) / 1e9, 2),
           "algorithmic_tb_per_s": round(rate / 1e12, 3), "fraction_of_8_tb_per_s": round(rate / HBM_BYTES_PER_S, 4)}
    rec.update(extra)
    print(json.dumps(rec), flush=True)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--skip-isa", action="store_true", help="do not compile csrc/bc7_kernels.hip for the instruction counts")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s, n = a.size, a.images
    strip = min(4, s)
    bad = False
    src_bytes, blk_bytes = n * s * s * 4, n * pkg.encoded_size(pkg.BC7, s, s)
    for name in ("noise", "smooth", "ramp"):
        img = B.content(name, s, s, 4)
        d1 = torch.from_numpy(img.reshape(-1).copy()).to(dev)
        d = d1.reshape(1, -1).repeat(n, 1)
        res = {}
        for leg, codec in (("bc7 encode", pkg.BC7), ("dxt5 encode", pkg.DXT5)):
            out = torch.empty((n, pkg.encoded_size(codec, s, s)), dtype=torch.uint8, device=dev)
            ms = time_launches(lambda: pkg.encode_device(codec, d, s, s, 4, n_images=n, out=out), a.k, a.reps, a.warmup)
            sse, _ = pkg.measure_error_device(codec, d1, out[0], s, s, 4)
            torch.cuda.synchronize()
            psnr = pkg.psnr_from_stats(sse[0].cpu().numpy(), s * s, 4)
            extra = {"psnr_rgba_db": round(psnr, 2), "kernel": pkg.kernel_name(codec, 4)}
            if codec == pkg.BC7:
                want = B.oracle_encode(img[:strip])
                ok = out[0].cpu().numpy()[:len(want)].tobytes() == want
                bad |= not ok
                extra["parity"] = "definition (image 0, first block row)" if ok else "MISMATCH"
                blocks = out
            res[leg] = (line(leg, name, n, s, ms, src_bytes + blk_bytes, **extra), psnr)
        pixels = torch.empty((n, s * s * 4), dtype=torch.uint8, device=dev)
        lib = pkg.lib()

        def decode():
            assert lib.icamd_decode_device(pkg.BC7, 0, s, s, 0, n, blocks.shape[1], s * s * 4, blocks.data_ptr(), pixels.data_ptr(),
                                           None) == 0
        ms = time_launches(decode, a.k, a.reps, a.warmup)
        ok = pixels[0, :strip * s * 4].cpu().numpy().tobytes() == B.decode(B.oracle_encode(img[:strip]), strip, s).tobytes()
        bad |= not ok
        line("bc7 decode", name, n, s, ms, src_bytes + blk_bytes, kernel="icamd_bc7_decode_kernel",
             parity="definition (image 0, first block row)" if ok else "MISMATCH")
        stats = torch.empty((n, pkg.ERROR_STATS_BYTES), dtype=torch.uint8, device=dev)
        ms = time_launches(lambda: pkg.measure_error_device(pkg.BC7, d, blocks, s, s, 4, n_images=n, out=stats), a.k, a.reps, a.warmup)
        line("bc7 metric", name, n, s, ms, src_bytes + blk_bytes, kernel=pkg.metric_kernel_name(pkg.BC7, 4))
        print(json.dumps({"comparison": "bc7 encode / dxt5 encode", "content": name,
                          "ratio_of_medians": round(res["bc7 encode"][0] / res["dxt5 encode"][0], 3),
                          "psnr_gain_db": round(res["bc7 encode"][1] - res["dxt5 encode"][1], 2)}), flush=True)
    counts = None if a.skip_isa else valu_per_block()
    print(json.dumps({"valu_instructions_per_block": counts if counts else "skipped" if a.skip_isa else "hipcc not available"}),
          flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
