#!/usr/bin/env python3
"""Device-resident cost and gain of BC6H's opt-in two-subset candidate (extension, include/ic_amd.h
icamd_encode_bc6h_modes_device): ICAMD_BC6H_MODES_EXTENDED next to ICAMD_BC6H_MODES_DEFAULT in the same run.

Per content (edge: two colour ramps per block across a straight edge, the gap cycling over 60 .. 14000 t-units; exponents,
gradient, ldr, flat: tests/bc6h_oracle.py) and format (UF16, SF16) at 16 x 4096^2 RGBA16F, one JSON line with
  ms per launch (median, min, max) of both, and EXTENDED / DEFAULT;
  the t-domain PSNR (peak 31743) of image 0 under both, from icamd_measure_error_bc6h_device;
  the share of image 0's blocks per mode field, counted from byte 0 of EXTENDED's output.
Once per run: the VGPR count and scratch size of the new kernels from the code object's metadata (hipcc -S; skipped without
hipcc or with --skip-isa; --isa-only prints that line alone and needs no GPU).  Parity: the first block row of image 0 against the
numpy definition (tests/bc6h_modes_oracle.py: test infrastructure, the checker only).
Method (scripts/bench_bc6h.py): untimed preconditioning calls, then device events around K back-to-back launches, repeated.
The content is generated at 1024^2 and tiled.

  python scripts/bench_bc6h_modes.py [--k 5] [--reps 5] [--size 4096] [--images 16] [--skip-isa | --isa-only]
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

CONTENTS = ("edge", "exponents", "gradient", "ldr", "flat")


def kernel_resources():
    """{kernel: {"vgprs", "sgprs", "scratch_bytes", "spilled_vgprs"}} of the new kernels from the compiler's metadata."""
    if not shutil.which("hipcc"):
        return None
    csrc = os.path.join(ROOT, "image-compression_amd", "csrc")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "bc6h_modes_kernels.s")
        subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-I" + csrc, "-S", "--cuda-device-only", "-o", asm, os.path.join(csrc, "bc6h_modes_kernels.hip")],
                              stderr=subprocess.DEVNULL)
        for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", open(asm).read(), re.S):
            blk = m.group(0)

            def field(key):
                return int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
            out[re.search(r"\.name:\s+(\S+)", blk).group(1)] = {
                "vgprs": field("vgpr_count"), "sgprs": field("sgpr_count"), "scratch_bytes": field("private_segment_fixed_size"),
                "spilled_vgprs": field("vgpr_spill_count")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--skip-isa", action="store_true", help="do not compile the kernels for the register and scratch figures")
    ap.add_argument("--isa-only", action="store_true", help="print the register and scratch figures alone (no GPU needed)")
    a = ap.parse_args()
    if a.isa_only:
        print(json.dumps({"kernel_resources": kernel_resources() or "hipcc not available"}), flush=True)
        return 0
    import numpy as np
    import torch

    import ic_amd_loader
    pkg = ic_amd_loader.load_package()
    import bc6h_modes_oracle as M

    def time_launches(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.k):
                fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / a.k)
        return out

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s, n = a.size, a.images
    strip = min(4, s)
    bad = False
    for name in CONTENTS:
        base = M.content(name, min(s, 1024), min(s, 1024), 4)
        reps = (s + base.shape[0] - 1) // base.shape[0]
        img = np.ascontiguousarray(np.tile(base, (reps, reps, 1))[:s, :s])
        d1 = torch.from_numpy(img.view(np.int16).reshape(-1)).to(dev).view(torch.float16)
        d = d1.reshape(1, -1).repeat(n, 1)
        for codec, signed, fmt in ((pkg.BC6H_UF16, False, "uf16"), (pkg.BC6H_SF16, True, "sf16")):
            blocks = torch.empty((n, pkg.encoded_size(codec, s, s)), dtype=torch.uint8, device=dev)
            rec = {"leg": "bc6h modes encode", "content": name, "format": fmt, "images": n, "size": s,
                   "kernel": pkg.bc6h_modes_kernel_name(codec, 4, pkg.BC6H_MODES_EXTENDED)}
            med = {}
            for label, modes in (("default", pkg.BC6H_MODES_DEFAULT), ("extended", pkg.BC6H_MODES_EXTENDED)):
                ms = time_launches(lambda: pkg.encode_bc6h_modes_device(codec, d, s, s, 4, bc6h_modes=modes, n_images=n, out=blocks))
                sse, _ = pkg.measure_error_bc6h_device(codec, d1, blocks[0], s, s, 4)
                torch.cuda.synchronize()
                med[label] = statistics.median(ms)
                rec["%s_ms_per_launch_median" % label] = round(med[label], 4)
                rec["%s_ms_min" % label], rec["%s_ms_max" % label] = round(min(ms), 4), round(max(ms), 4)
                rec["%s_psnr_t_domain_db" % label] = round(pkg.psnr_bc6h_from_stats(sse[0].cpu().numpy(), s * s), 2)
                want = M.oracle_encode(img[:strip], signed, modes=modes)
                ok = blocks[0].cpu().numpy()[:len(want)].tobytes() == want
                bad |= not ok
                rec["%s_parity" % label] = "definition (image 0, first block row)" if ok else "MISMATCH"
            # (blocks now holds EXTENDED's output)
            b0 = blocks[0][::16].to(torch.int64)
            fields = torch.where((b0 & 3) < 2, b0 & 3, b0 & 31)
            counts = torch.bincount(fields, minlength=32).cpu().numpy()
            rec["extended_over_default"] = round(med["extended"] / med["default"], 3)
            rec["mode_field_share"] = {format(f, "02b" if f < 2 else "05b"): round(float(c) / len(b0), 4)
                                       for f, c in enumerate(counts) if c}
            print(json.dumps(rec), flush=True)
    res = None if a.skip_isa else kernel_resources()
    print(json.dumps({"kernel_resources": res if res else "skipped" if a.skip_isa else "hipcc not available"}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
