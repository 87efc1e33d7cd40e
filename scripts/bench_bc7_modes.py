#!/usr/bin/env python3
"""Device-resident throughput and quality of BC7's opt-in mode-1 / mode-5 candidates (extension, include/ic_amd.h
ICAMD_BC7_MODES_EXTENDED) against the mode-6 encoder (ICAMD_BC7_MODES_DEFAULT) in the same run.

Per source format (RGBA8, RGB888) and content (noise, smooth, ramp of tests/bc7_oracle.py; edge: two shaded regions meeting
along a stepped edge, tests/bc7_modes_oracle.py) at 16 x 4096^2:
  default, extended   icamd_encode_bc7_device; ms per launch as median (min - max), the PSNR of image 0 from
                      icamd_measure_error_device, the share of blocks of image 0 in modes 1 / 5 / 6 read from byte 0, a sha256
                      of image 0's blocks;
  one comparison line the ratio of the medians, the PSNR gain.
Parity: a 64 x 60 image (the mixed wave of the tests for RGBA8, the edge content for RGB888) against the numpy definition
(tests/bc7_modes_oracle.py: test infrastructure, the checker only).  One line reports the VALU instructions of the kernels from
the compiler's ISA (skipped without hipcc).
--default-only times icamd_encode_device(ICAMD_BC7) alone, so that the same script runs against a library that predates the
entry point (an A/B of the DEFAULT path: compare the sha256 and the medians of two runs).
Method (scripts/bench_bc7.py): untimed preconditioning calls, then device events around K back-to-back launches, repeated.

  python scripts/bench_bc7_modes.py [--k 5] [--reps 5] [--size 4096] [--images 16] [--skip-isa] [--default-only]
Exit status 1 if any parity fails."""
import argparse
import hashlib
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
import torch  # noqa: E402

import ic_amd_loader  # noqa: E402

pkg = ic_amd_loader.load_package()
import bc7_modes_oracle as M  # noqa: E402
import bc7_oracle as B  # noqa: E402


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
    """{kernel: (VALU instructions, of them dot products, VGPRs)} from the compiler's ISA: static counts, one block per lane."""
    if not shutil.which("hipcc"):
        return None
    csrc = os.path.join(ROOT, "image-compression_amd", "csrc")
    counts = {}
    with tempfile.TemporaryDirectory() as tmp:
        for unit, names in (("bc7_kernels", ("icamd_bc7_rgba8_kernel", "icamd_bc7_rgb888_kernel")),
                            ("bc7_modes_kernels", ("icamd_bc7_modes_rgba8_kernel", "icamd_bc7_modes_rgb888_kernel"))):
            out = os.path.join(tmp, unit + ".s")
            subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                                   "-I" + csrc, "-S", "--cuda-device-only", "-o", out, os.path.join(csrc, unit + ".hip")],
                                  stderr=subprocess.DEVNULL)
            text = open(out).read()
            for name in names:
                body = text[text.index("\n%s:" % name):]
                body = body[:body.index("s_endpgm")]
                vgprs = int(re.search(r"\.name:\s+%s\n.*?\.vgpr_count:\s+(\d+)" % name, text, re.S).group(1))
                counts[name] = {"valu": len(re.findall(r"^\s+v_\w+", body, re.M)), "dot4": len(re.findall(r"^\s+v_dot4", body, re.M)),
                                "vgprs": vgprs}
    return counts


def image(name, s, comps):
    return M.stepped_edge_image(s, s, comps) if name == "edge" else B.content(name, s, s, comps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--skip-isa", action="store_true", help="do not compile the kernels for the instruction counts")
    ap.add_argument("--default-only", action="store_true", help="time icamd_encode_device(ICAMD_BC7) alone")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    s, n = a.size, a.images
    bad = False
    if not a.default_only:
        for comps, img in ((4, M.modes_wave_image()[0][:64, :60].copy()), (3, M.stepped_edge_image(64, 60, 3))):
            got = pkg.encode_bc7_device(torch.from_numpy(img.reshape(-1).copy()).to(dev), 64, 60, comps, bc7_modes=pkg.BC7_MODES_EXTENDED)
            torch.cuda.synchronize()
            ok = got.cpu().numpy().tobytes() == M.oracle_encode(img)
            bad |= not ok
            print(json.dumps({"parity": "definition (64 x 60, %d components)" % comps, "ok": ok}), flush=True)
    for comps in (4, 3):
        for name in ("noise", "smooth", "ramp", "edge"):
            d1 = torch.from_numpy(image(name, s, comps).reshape(-1)).to(dev)
            d = d1.reshape(1, -1).repeat(n, 1)
            out = torch.empty((n, pkg.encoded_size(pkg.BC7, s, s)), dtype=torch.uint8, device=dev)
            res = {}
            for leg, modes in (("default", 0),) if a.default_only else (("default", 0), ("extended", 1)):
                if a.default_only:
                    fn = lambda: pkg.encode_device(pkg.BC7, d, s, s, comps, n_images=n, out=out)  # noqa: E731
                    kernel = pkg.kernel_name(pkg.BC7, comps)
                else:
                    fn = lambda: pkg.encode_bc7_device(d, s, s, comps, bc7_modes=modes, n_images=n, out=out)  # noqa: E731
                    kernel = pkg.bc7_kernel_name(comps, modes)
                ms = time_launches(fn, a.k, a.reps, a.warmup)
                sse, _ = pkg.measure_error_device(pkg.BC7, d1, out[0], s, s, comps)
                torch.cuda.synchronize()
                psnr = pkg.psnr_from_stats(sse[0].cpu().numpy(), s * s, comps)
                blocks = out[0].cpu().numpy()
                b0 = blocks.reshape(-1, 16)[:, 0]
                share = {m: round(float(((b0 & ((2 << m) - 1)) == (1 << m)).mean()), 4) for m in (1, 5, 6)}
                m = statistics.median(ms)
                res[leg] = (m, psnr)
                print(json.dumps({"leg": leg, "components": comps, "content": name, "images": n, "size": s, "kernel": kernel,
                                  "ms_per_launch_median": round(m, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                                  "gpixels_per_s": round(n * s * s / (m * 1e-3) / 1e9, 2), "psnr_db": round(psnr, 2),
                                  "share_of_blocks_by_mode": share, "sha256_image0": hashlib.sha256(blocks.tobytes()).hexdigest()[:16]}),
                      flush=True)
            if not a.default_only:
                print(json.dumps({"comparison": "extended / default", "components": comps, "content": name,
                                  "ratio_of_medians": round(res["extended"][0] / res["default"][0], 3),
                                  "psnr_gain_db": round(res["extended"][1] - res["default"][1], 2)}), flush=True)
    counts = None if a.skip_isa else valu_counts()
    print(json.dumps({"static_instruction_counts": counts if counts else "skipped" if a.skip_isa else "hipcc not available"}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
