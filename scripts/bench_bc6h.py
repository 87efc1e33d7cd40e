#!/usr/bin/env python3
"""Device-resident throughput and quality of BC6H (extension, include/ic_amd.h icamd_encode_bc6h_device) next to
BC7's default (mode 6) encoder in the same run.

Per content (exponents: every block spans 20 binary exponents, random mantissas, one sample in eight negative; gradient: a smooth
HDR gradient from 2^-6 to 2^12; ldr: linear ramps in [0, 1]) and format (UF16, SF16) at 16 x 4096^2 RGBA16F:
  bc6h encode    icamd_encode_bc6h_device; ms per launch (median, min, max), the t-domain PSNR (peak 31743) of image 0 from
                 icamd_measure_error_bc6h_device, algorithmic bytes (source read + blocks written, once each) per second and their
                 fraction of 8 TB/s;
  bc6h decode, bc6h metric   icamd_decode_bc6h_device / icamd_measure_error_bc6h_device on the encoder's blocks, timed the same way.
Once per run: bc7 encode (icamd_encode_bc7_device, BC7_MODES_DEFAULT, 16 x 4096^2 RGBA8 noise) and the ratio of every BC6H encode
median to it; the VALU instructions of the BC6H kernels from the compiler's ISA (hipcc -S; skipped without hipcc; the index
search is a rolled loop of 16 iterations, counted once in the static figure).  Parity: the first block row of image 0 against the
numpy definition (tests/bc6h_oracle.py: test infrastructure, the checker only).
Method (scripts/bench_bc7.py): untimed preconditioning calls, then device events around K back-to-back launches, repeated.
The content is generated at 1024^2 and tiled.

  python scripts/bench_bc6h.py [--k 5] [--reps 5] [--size 4096] [--images 16] [--skip-isa]
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
import bc6h_oracle as B  # noqa: E402
import bc7_oracle as B7  # noqa: E402

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


def valu_counts():
    """{kernel: (instructions, VALU instructions, of which 32-bit multiplies) in its ISA} -- static counts."""
    if not shutil.which("hipcc"):
        return None
    csrc = os.path.join(ROOT, "image-compression_amd", "csrc")
    counts = {}
    with tempfile.TemporaryDirectory() as tmp:
        for unit, names in (("bc6h_kernels", ("icamd_bc6h_uf16_rgba16f_kernel", "icamd_bc6h_sf16_rgba16f_kernel",
                                              "icamd_bc6h_uf16_decode_kernel", "icamd_metric_bc6h_uf16_rgba16f_kernel")),
                            ("bc7_kernels", ("icamd_bc7_rgba8_kernel",))):
            out = os.path.join(tmp, unit + ".s")
            subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                                   "-I" + csrc, "-S", "--cuda-device-only", "-o", out, os.path.join(csrc, unit + ".hip")],
                                  stderr=subprocess.DEVNULL)
            text = open(out).read()
            for name in names:
                body = text[text.index("\n%s:" % name):]
                body = body[:body.index("s_endpgm")]
                counts[name] = {"instructions": len(re.findall(r"^\s+[sv]_\w+|^\s+(?:global|ds|buffer|flat|scratch)_\w+", body, re.M)),
                                "valu": len(re.findall(r"^\s+v_\w+", body, re.M)),
                                "mul_32": len(re.findall(r"^\s+v_(?:mul_lo|mul_hi|mad_u64|mad_i64)\w+", body, re.M))}
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


def tiled(img, s):
    reps = (s + img.shape[0] - 1) // img.shape[0]
    return np.ascontiguousarray(np.tile(img, (reps, reps, 1))[:s, :s])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--skip-isa", action="store_true", help="do not compile the kernels for the instruction counts")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s, n = a.size, a.images
    strip = min(4, s)
    bad = False
    lib = pkg.lib()
    # BC7 mode 6, the closest existing kernel, in the same run
    img8 = tiled(B7.content("noise", min(s, 1024), min(s, 1024), 4), s)
    d8 = torch.from_numpy(img8.reshape(-1)).to(dev).reshape(1, -1).repeat(n, 1)
    out8 = torch.empty((n, pkg.encoded_size(pkg.BC7, s, s)), dtype=torch.uint8, device=dev)
    ms = time_launches(lambda: pkg.encode_bc7_device(d8, s, s, 4, bc7_modes=pkg.BC7_MODES_DEFAULT, n_images=n, out=out8), a.k, a.reps,
                       a.warmup)
    bc7_ms = line("bc7 encode (DEFAULT)", "noise", n, s, ms, n * s * s * 4 + out8.numel(), kernel=pkg.kernel_name(pkg.BC7, 4))
    del d8, out8
    src_bytes, blk_bytes = n * s * s * 8, n * pkg.encoded_size(pkg.BC6H_UF16, s, s)
    for name in ("exponents", "gradient", "ldr"):
        img = tiled(B.content(name, min(s, 1024), min(s, 1024), 4), s)
        d1 = torch.from_numpy(img.view(np.int16).reshape(-1)).to(dev).view(torch.float16)
        d = d1.reshape(1, -1).repeat(n, 1)
        for codec, signed, fmt in ((pkg.BC6H_UF16, False, "uf16"), (pkg.BC6H_SF16, True, "sf16")):
            blocks = torch.empty((n, pkg.encoded_size(codec, s, s)), dtype=torch.uint8, device=dev)
            ms = time_launches(lambda: pkg.encode_bc6h_device(codec, d, s, s, 4, n_images=n, out=blocks), a.k, a.reps, a.warmup)
            sse, _ = pkg.measure_error_bc6h_device(codec, d1, blocks[0], s, s, 4)
            torch.cuda.synchronize()
            psnr = pkg.psnr_bc6h_from_stats(sse[0].cpu().numpy(), s * s)
            want = B.oracle_encode(img[:strip], signed)
            ok = blocks[0].cpu().numpy()[:len(want)].tobytes() == want
            bad |= not ok
            m = line("bc6h encode", name, n, s, ms, src_bytes + blk_bytes, format=fmt, psnr_t_domain_db=round(psnr, 2),
                     kernel=pkg.bc6h_kernel_name(codec, 4), ratio_to_bc7_default=round(statistics.median(ms) / bc7_ms, 3),
                     parity="definition (image 0, first block row)" if ok else "MISMATCH")
            del m
            pixels = torch.empty((n, s * s * 8), dtype=torch.uint8, device=dev)

            def decode():
                assert lib.icamd_decode_bc6h_device(codec, s, s, 0, n, blocks.shape[1], s * s * 8, blocks.data_ptr(),
                                                    pixels.data_ptr(), None) == 0
            ms = time_launches(decode, a.k, a.reps, a.warmup)
            ok = pixels[0, :strip * s * 8].cpu().numpy().tobytes() == B.decode(want, strip, s, signed).tobytes()
            bad |= not ok
            line("bc6h decode", name, n, s, ms, src_bytes + blk_bytes, format=fmt, kernel="icamd_bc6h_%s_decode_kernel" % fmt,
                 parity="definition (image 0, first block row)" if ok else "MISMATCH")
            del pixels
            stats = torch.empty((n, pkg.ERROR_STATS_BYTES), dtype=torch.uint8, device=dev)
            ms = time_launches(lambda: pkg.measure_error_bc6h_device(codec, d, blocks, s, s, 4, n_images=n, out=stats), a.k, a.reps,
                               a.warmup)
            line("bc6h metric", name, n, s, ms, src_bytes + blk_bytes, format=fmt, kernel=pkg.bc6h_kernel_name(codec, 4, metric=True))
    counts = None if a.skip_isa else valu_counts()
    print(json.dumps({"static_instruction_counts": counts if counts else "skipped" if a.skip_isa else "hipcc not available"}),
          flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
