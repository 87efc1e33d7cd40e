"""CPU tier: the status (and, when negative, the icamd_last_error() text) of every argument-checking C entry point over
a fixed grid of argument variations, pinned to tests/golden/capi_statuses.json.

On a machine without a HIP device every call that passes validation stops at require_device() with ICAMD_ERR_NO_DEVICE,
so the table pins the outcome and the order of every check that runs before the device is touched.  The device pointers
are dummy addresses: the test skips where a device is visible (a call that passes validation would launch on them).
Host buffers that an entry point really reads or writes before the device check are real numpy arrays.

Regenerate the table from a build of the library with `python tests/test_capi_statuses.py`."""
import ctypes
import itertools
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "capi_statuses.json")

# entry points whose result is a size or a count, not a status: recorded as plain numbers
SIZE_RESULTS = {"icamd_compute_compressed_data_size", "icamd_supports_format", "icamd_encoded_size",
                "icamd_pvrtc2_workspace_size", "icamd_pvrtc4_workspace_size", "icamd_container_size", "icamd_mip_max_levels",
                "icamd_mip_chain_size", "icamd_mip_workspace_size", "icamd_wall_clock_rate_khz", "icamd_device_count"}

# dummy device addresses: aligned to 256, and 1, 4 and 8 bytes past that; N = NULL
A, M1, M4, M8, N = 0x100000, 0x100001, 0x100004, 0x100008, 0
CODECS = list(range(-1, 8))       # DXT1 .. BC5 and one out of range on each side
COMPRESSORS = list(range(-1, 4))  # DXTC, ETC, PVRTC and one out of range on each side
FORMATS = list(range(-1, 5))      # RGB .. BGRA and one out of range on each side
COMPS = list(range(0, 6))
SIZES = [(0, 8), (8, 0), (1, 1), (3, 3), (7, 7), (8, 8), (64, 64), (32768, 32768), (65536, 65536), (8, 16), (16, 8),
         (12, 20), (24, 24)]
SMALL = [(0, 8), (1, 1), (3, 3), (7, 7), (8, 8), (64, 64), (8, 16), (12, 20)]  # host outputs really written
BIG = 1 << 40
SQUARES = [0, 1, 3, 7, 8, 12, 64, 32768, 65536]


def b4(n):
    return (n + 3) // 4


def fmt_comps(fmt):
    return 3 if fmt in (0, 1) else 4 if fmt in (2, 3) else 0


def mip_max(h, w):
    return max(h, w).bit_length() if h and w else 0


def levels_of(h, w):
    """levels 0, 1, the maximum and one past it"""
    return [0, 1, mip_max(h, w), mip_max(h, w) + 1]


class Lib:
    def __init__(self, pkg):
        """a library handle of its own, with the package's prototypes (image-compression_amd/abi.py)"""
        self.L = pkg.abi.bind(ctypes.CDLL(pkg.LIB_PATH))
        self.keep = []  # host buffers of the current call

    def __getattr__(self, name):
        return getattr(self.L, name)

    def buf(self, nbytes, dtype=np.uint8):
        """a real host buffer of at least nbytes, kept alive for the call"""
        a = np.zeros(max(int(nbytes), 1), dtype)
        self.keep.append(a)
        return a.ctypes.data

    def array(self, values, dtype):
        a = np.array(values, dtype)
        self.keep.append(a)
        return a.ctypes.data

    def ptrs(self, addrs):
        a = (ctypes.c_void_p * max(len(addrs), 1))(*addrs)
        self.keep.append(a)
        return ctypes.addressof(a)

    def ints(self, values):
        a = (ctypes.c_int * max(len(values), 1))(*values)
        self.keep.append(a)
        return ctypes.addressof(a)


def grid(lib):
    """Yields (entry point, argument tuple) in a fixed order.  Arguments that are callables get the library (host buffers
    built per call)."""
    C = lib  # (sizes that the grids compute from the library's own queries)

    for comp, fmt, (h, w) in itertools.product(COMPRESSORS, FORMATS, SIZES):
        yield "icamd_compute_compressed_data_size", (comp, fmt, h, w)
    for comp, fmt in itertools.product(COMPRESSORS, FORMATS):
        yield "icamd_supports_format", (comp, fmt)
    for codec, (h, w) in itertools.product(CODECS, SIZES):
        yield "icamd_encoded_size", (codec, h, w)
    for size, n in itertools.product(SQUARES, [0, 1, 2]):
        yield "icamd_pvrtc2_workspace_size", (size, n)
        yield "icamd_pvrtc4_workspace_size", (size, n)
    for cont, codec, (h, w) in itertools.product(range(-1, 5), CODECS, [(0, 8), (1, 1), (8, 8), (64, 64), (12, 20),
                                                                         (65536, 65536)]):
        for levels in levels_of(h, w) + [33]:
            yield "icamd_container_size", (cont, codec, h, w, levels)

    # container_write: level views and output are real buffers
    def container_args(cont, codec, h, w, levels, variant):
        def make(lib):
            need = C.icamd_container_size(cont, codec, h, w, levels)
            sizes = [C.icamd_encoded_size(codec, max(1, h >> l), max(1, w >> l)) for l in range(levels)] + [0] * 33
            if variant == "wrong_level":
                sizes[levels - 1] += 8
            data = lib.buf(max(sizes) + 8)
            level_data = lib.ptrs([data] * 33)
            level_sizes = lib.array(sizes[:33], np.uint64)
            out_size = need + 1 if variant == "long_out" else need
            return (cont, codec, h, w, levels, N if variant == "null_data" else level_data,
                    N if variant == "null_sizes" else level_sizes, N if variant == "null_out" else lib.buf(out_size + 1),
                    out_size)
        return make
    for cont, codec, (h, w, levels) in itertools.product(range(-1, 5), CODECS, [(8, 8, 1), (64, 64, 7), (64, 64, 4),
                                                                               (12, 20, 1)]):
        for variant in ["ok", "long_out", "wrong_level"]:
            yield "icamd_container_write", container_args(cont, codec, h, w, levels, variant)
    for variant in ["null_data", "null_sizes", "null_out"]:
        yield "icamd_container_write", container_args(0, 0, 8, 8, 1, variant)

    # ---- device encode
    for codec, comps, swap, (h, w) in itertools.product(CODECS, COMPS, [0, 1], SIZES):
        stride = w * max(comps, 1)
        yield "icamd_encode_device", (codec, 2, comps, swap, h, w, h, w, stride, 1, 0, 0, A, A, N)
    for codec, comps, (h, w), rs, n in itertools.product(CODECS, [1, 3, 4], [(8, 8), (64, 64)], ["exact", "short", "rgba"],
                                                         [0, 1, 2]):
        stride = {"exact": w * comps, "short": w * comps - 1, "rgba": w * 4}[rs]
        yield "icamd_encode_device", (codec, 2, comps, 0, h, w, h, w, stride, n, h * stride, b4(h) * b4(w) * 16, A, A, N)
    for codec, comps, n, (src, dst), (ss, ds) in itertools.product(
            CODECS, [2, 4], [1, 2], [(N, A), (A, N), (M1, A), (M8, A), (A, M4), (M4, M8)],
            [(0, 0), (16384, 2048), (16388, 2048), (16384, 2052)]):
        yield "icamd_encode_device", (codec, 2, comps, 0, 64, 64, 64, 64, 64 * comps, n, ss, ds, src, dst, N)
    for size, first, nb, (src, dst) in itertools.product(SQUARES, [0, 2, 3], [0, 1, 2, 3, 4, 128, 256],
                                                         [(A, A), (N, A), (A, N), (M8, A), (A, M4)]):
        yield "icamd_pvrtc2_encode_region_device", (size, first, nb, src, dst, N)

    # ---- Compressor::Compress / CompressAndPad, device and host buffers (nothing is touched before the device check)
    for comp, fmt, (h, w), pad, long_out in itertools.product(COMPRESSORS, FORMATS, SIZES, [0, 4], [0, 1]):
        out = C.icamd_compute_compressed_data_size(comp, fmt, h, w) + long_out
        yield "icamd_compress_device", (comp, 2, fmt, h, w, pad, A, A, out, N)
        yield "icamd_compress", (comp, 2, fmt, h, w, pad, A, A, out)
    for comp, fmt, (src, dst) in itertools.product(COMPRESSORS, [0, 2], [(N, A), (A, N), (M1, M1)]):
        yield "icamd_compress_device", (comp, 2, fmt, 8, 8, 0, src, dst, C.icamd_compute_compressed_data_size(comp, fmt, 8, 8), N)
        yield "icamd_compress", (comp, 2, fmt, 8, 8, 0, src, dst, C.icamd_compute_compressed_data_size(comp, fmt, 8, 8))
    for comp, fmt, (h, w), (dh, dw), pad, long_out in itertools.product(
            [-1, 0, 1, 2], [-1, 0, 2, 3], [(0, 8), (7, 7), (8, 8), (64, 64), (12, 20)], [(0, 0), (8, 4), (-4, -4)], [0, 4],
            [0, 1]):
        ph, pw = max(h + dh, 0), max(w + dw, 0)
        out = C.icamd_compute_compressed_data_size(comp, fmt, max(h, ph), max(w, pw)) + long_out
        yield "icamd_compress_and_pad_device", (comp, 2, fmt, h, w, ph, pw, pad, A, A, out, N)
        yield "icamd_compress_and_pad", (comp, 2, fmt, h, w, ph, pw, pad, A, A, out)

    # ---- decode
    for codec, swap, (h, w), pad, n in itertools.product(CODECS, [0, 1], SIZES, [0, 4], [0, 1]):
        yield "icamd_decode_device", (codec, swap, h, w, pad, n, 0, 0, A, A, N)
    for codec, (src, dst) in itertools.product(CODECS, [(N, A), (A, N)]):
        yield "icamd_decode_device", (codec, 0, 8, 8, 0, 1, 0, 0, src, dst, N)
    for comp, fmt, (h, w), pad, long_in, long_out in itertools.product([-1, 0, 1, 2], [-1, 0, 1, 2, 3], SMALL, [0, 4], [0, 1],
                                                                       [0, 1]):
        blocks = C.icamd_compute_compressed_data_size(comp, fmt, h, w) + long_in
        out = h * (w * fmt_comps(fmt) + pad) + long_out
        yield "icamd_decompress", (comp, fmt, h, w, pad, A, blocks, A, out)
    for comp, (src, dst) in itertools.product([0, 1], [(N, A), (A, N)]):
        yield "icamd_decompress", (comp, 0, 8, 8, 0, src, 32, dst, 192)
    for size, long_in, long_out, (src, dst) in itertools.product(SQUARES, [0, 1], [0, 1], [(A, A), (N, A), (A, N)]):
        yield "icamd_pvrtc2_decompress", (size, src, size * size // 4 + long_in, dst, size * size * 4 + long_out)

    # ---- compressed-domain operations
    def blockop_size(comp, fmt, h, w):
        return C.icamd_compute_compressed_data_size(comp, fmt, h, w) if comp in (0, 1) else 0

    PAD_SIZES = [(0, 8), (7, 7), (8, 8), (64, 64), (12, 20)]
    for comp, fmt, (h, w), (dh, dw), long_out in itertools.product([-1, 0, 1, 2], [-1, 0, 2], PAD_SIZES,
                                                                   [(0, 0), (8, 4), (-4, 0)], [0, 1]):
        ph, pw = max(h + dh, 0), max(w + dw, 0)
        out = blockop_size(comp, fmt, ph, pw) + long_out
        yield "icamd_pad_batch_device", (comp, 2, fmt, h, w, 1, A, 0, ph, pw, A, 0, out, N)
        yield "icamd_pad_device", (comp, 2, fmt, h, w, A, ph, pw, A, out, N)
        yield "icamd_pad", (comp, 2, fmt, h, w, A, ph, pw, A, out)
    for comp, fmt, n, strides, (src, dst) in itertools.product(
            [0, 1], [0, 2], [0, 1, 2], ["zero", "exact", "short_src", "short_dst", "odd"], [(A, A), (M1, A), (A, M1), (N, A)]):
        si, so = blockop_size(comp, fmt, 12, 20), blockop_size(comp, fmt, 16, 24)
        ss, ds = {"zero": (0, 0), "exact": (si, so), "short_src": (si - 8, so), "short_dst": (si, so - 8),
                  "odd": (si + 2, so)}[strides]
        yield "icamd_pad_batch_device", (comp, 2, fmt, 12, 20, n, src, ss, 16, 24, dst, ds, so, N)
    DS_SIZES = [(0, 8), (1, 1), (3, 3), (3, 8), (7, 7), (8, 8), (12, 12), (16, 8), (64, 64), (12, 20), (24, 24)]
    for comp, fmt, (h, w), long_out in itertools.product([-1, 0, 1, 2], [-1, 0, 2], DS_SIZES, [0, 1]):
        out = blockop_size(comp, fmt, (h + 1) // 2, (w + 1) // 2) + long_out
        yield "icamd_downsample_batch_device", (comp, 2, fmt, h, w, 1, A, 0, A, 0, out, N)
        yield "icamd_downsample_device", (comp, 2, fmt, h, w, A, A, out, N)
        yield "icamd_downsample", (comp, 2, fmt, h, w, A, A, out)
    for comp, fmt, n, strides, (src, dst) in itertools.product(
            [0, 1], [0, 2], [0, 1, 2], ["zero", "exact", "short_src", "short_dst", "odd"], [(A, A), (M1, A), (A, M1), (N, A)]):
        si, so = blockop_size(comp, fmt, 16, 24), blockop_size(comp, fmt, 8, 12)
        ss, ds = {"zero": (0, 0), "exact": (si, so), "short_src": (si - 8, so), "short_dst": (si, so - 8),
                  "odd": (si, so + 2)}[strides]
        yield "icamd_downsample_batch_device", (comp, 2, fmt, 16, 24, n, src, ss, dst, ds, so, N)
    for ptr, nbytes in itertools.product([N, A, M4, M8], [0, 7, 8, 12, 64]):
        yield "icamd_transcode_dxt1_to_etc1_device", (ptr, nbytes, N)
    for ptr, nbytes in itertools.product([N, A], [0, 7, 8, 12, 64]):
        yield "icamd_transcode_dxt1_to_etc1", (ptr, nbytes)

    # ---- CreateSolidImage / CopySubimage
    def solid_size(comp, fmt, h, w):
        bb = 8 if (comp == 0 and fmt in (0, 1)) or (comp == 1 and fmt == 0) else 16 if comp == 0 and fmt in (2, 3) else 0
        return b4(h) * b4(w) * bb

    def with_colors(name, args):
        def make(lib):
            return tuple(lib.buf(16) if a == "colors" else a for a in args)
        return name, make
    SOLID_SIZES = SMALL + [(65536, 65536), (1 << 20, 1 << 20)]
    for comp, fmt, (h, w), long_out in itertools.product([-1, 0, 1, 2], [-1, 0, 1, 2, 3], SOLID_SIZES, [0, 1]):
        out = solid_size(comp, fmt, h, w) + long_out
        yield with_colors("icamd_create_solid_batch_device", (comp, fmt, h, w, 1, "colors", A, 0, out, N))
        yield with_colors("icamd_create_solid_device", (comp, fmt, h, w, "colors", A, out, N))
    for n, ds, (colors, dst) in itertools.product([0, 1, 2], [0, 64, 32, 66], [("colors", A), ("colors", M1), ("colors", N),
                                                                               (N, A)]):
        yield with_colors("icamd_create_solid_batch_device", (0, 2, 8, 8, n, colors, dst, ds, 64, N))
    for comp, fmt, (h, w), long_out in itertools.product([-1, 0, 1, 2], [-1, 0, 1, 2, 3], SMALL, [0, 1]):
        out = solid_size(comp, fmt, h, w) + long_out

        def make(lib, comp=comp, fmt=fmt, h=h, w=w, out=out):
            return (comp, fmt, h, w, lib.buf(16), lib.buf(out), out)
        yield "icamd_create_solid", make
    for colors, dst in [(N, "out"), ("colors", N)]:
        yield with_colors("icamd_create_solid", (0, 0, 8, 8, colors, A if dst == "out" else N, 32))

    WINDOWS = [(0, 0, 4, 4), (4, 4, 4, 4), (2, 0, 4, 4), (0, 0, 3, 4), (0, 0, 64, 64), (60, 60, 8, 8),
               (0xfffffffc, 0, 8, 4)]
    for comp, fmt, (ch, cw), (r, c, h, w), long_out in itertools.product([-1, 0, 1, 2], [-1, 0, 2], [(8, 8), (64, 64)],
                                                                         WINDOWS, [0, 1]):
        out = solid_size(comp, 2 if fmt == 2 else fmt, h, w) + long_out
        yield "icamd_copy_subimage_batch_device", (comp, fmt, ch, cw, 1, A, 0, r, c, h, w, A, 0, out, N)
        yield "icamd_copy_subimage_device", (comp, fmt, ch, cw, A, r, c, h, w, A, out, N)

        def make(lib, comp=comp, fmt=fmt, ch=ch, cw=cw, r=r, c=c, h=h, w=w, out=out):
            return (comp, fmt, ch, cw, lib.buf(b4(ch) * b4(cw) * 16), r, c, h, w, lib.buf(out), out)
        yield "icamd_copy_subimage", make
    for n, strides, (src, dst) in itertools.product([0, 1, 2], ["zero", "exact", "short_src", "short_dst", "odd"],
                                                    [(A, A), (M1, A), (A, M1), (N, A)]):
        ss, ds = {"zero": (0, 0), "exact": (256, 64), "short_src": (248, 64), "short_dst": (256, 56), "odd": (258, 64)}[strides]
        yield "icamd_copy_subimage_batch_device", (0, 2, 16, 16, n, src, ss, 4, 4, 8, 8, dst, ds, 64, N)

    # ---- multi-GPU batches (the device list is read only after the device check)
    def batch_args(name, n, lists, n_devices, h=8):
        def make(lib):
            devs = lib.ints([0] * 300)
            stats = lib.ints([0] * 4)
            if name == "icamd_compress_batch":
                bufs, outs = lib.ptrs([A, A]), lib.ptrs([A, A])
                return (0, 2, 0, h, 8, 0, n, N if lists == "null_src" else bufs, N if lists == "null_dst" else outs, 32,
                        N if lists == "null_devices" else devs, n_devices, stats)
            srcs, dsts = lib.ptrs([A, A]), lib.ptrs([A, A])
            gather = 0 if lists in ("gather", "gather_null_buf") else -1
            return (0, 2, 4, 0, h, 8, 32, n, N if lists == "null_src" else srcs,
                    N if lists in ("null_dst", "gather") else dsts, N if lists == "null_devices" else devs, n_devices, gather,
                    N if lists == "gather_null_buf" else A, 64, stats)
        return make
    for n, lists, n_devices in itertools.product([0, 1, 2], ["ok", "null_src", "null_dst", "null_devices"],
                                                 [-1, 0, 1, 256, 257]):
        yield "icamd_compress_batch", batch_args("icamd_compress_batch", n, lists, n_devices)
    for n, lists, n_devices, h in itertools.product([0, 1, 2], ["ok", "null_src", "null_dst", "null_devices", "gather",
                                                                "gather_null_buf"], [0, 1, 257], [0, 8]):
        yield "icamd_encode_batch_sharded_device", batch_args("icamd_encode_batch_sharded_device", n, lists, n_devices, h)

    # ---- mip chains
    for h, w in SIZES + [(1, 65536), (5, 3)]:
        yield "icamd_mip_max_levels", (h, w)
    for codec, (h, w) in itertools.product(CODECS, SIZES):
        for levels in levels_of(h, w):
            yield "icamd_mip_chain_size", (lambda lib, a=(codec, h, w, levels): a + (lib.buf(8 * 34),))
    for codec, comps, (h, w), n in itertools.product([0, 2, 3, 5, 7], [0, 1, 3, 5], [(0, 8), (64, 64), (12, 20),
                                                                                      (65536, 65536)], [1, 2]):
        for levels in levels_of(h, w):
            yield "icamd_mip_workspace_size", (codec, comps, h, w, levels, n)
    for codec, comps, swap, (h, w) in itertools.product(CODECS, COMPS, [0, 1], [(8, 8), (0, 8), (256, 256)]):
        for levels in [0, mip_max(h, w), mip_max(h, w) + 1]:
            yield "icamd_encode_mips_device", (codec, 2, comps, swap, h, w, w * max(comps, 1), levels, 1, 0, 0, A, A, A, BIG, N)
    for codec, comps, rs, n, strides, ws in itertools.product(
            [0, 2, 5, 6], [2, 4], ["exact", "short"], [0, 1, 2], ["zero", "exact", "short_src", "short_dst"],
            ["ok", "null", "short"]):
        stride = 256 * comps - (1 if rs == "short" else 0)
        src = 255 * stride + 256 * comps
        chain = C.icamd_mip_chain_size(codec, 256, 256, 9, None)
        need = C.icamd_mip_workspace_size(codec, comps, 256, 256, 9, n)
        ss, ds = {"zero": (0, 0), "exact": (src, chain), "short_src": (src - 1, chain), "short_dst": (src, chain - 8)}[strides]
        wp, wb = {"ok": (A, need), "null": (N, need), "short": (A, max(need, 1) - 1)}[ws]
        yield "icamd_encode_mips_device", (codec, 2, comps, 0, 256, 256, stride, 9, n, ss, ds, A, A, wp, wb, N)
    for codec, (src, dst) in itertools.product([0, 2], [(N, A), (A, N)]):
        yield "icamd_encode_mips_device", (codec, 2, 4, 0, 8, 8, 32, 4, 1, 0, 0, src, dst, A, BIG, N)
    for comps, (h, w) in itertools.product(COMPS, [(8, 8), (0, 8), (256, 256), (12, 20)]):
        for levels in levels_of(h, w):
            yield "icamd_mip_pyramid_device", (comps, h, w, w * max(comps, 1), levels, 1, 0, 0, A, A, N)
    for comps, rs, n, strides, (src, dst) in itertools.product([1, 4], ["exact", "short"], [0, 1, 2],
                                                               ["zero", "exact", "short_src", "short_dst"],
                                                               [(A, A), (N, A), (A, N)]):
        stride = 256 * comps - (1 if rs == "short" else 0)
        sb = 255 * stride + 256 * comps
        per = sum(max(1, 256 >> l) ** 2 * comps for l in range(1, 9))
        ss, ds = {"zero": (0, 0), "exact": (sb, per), "short_src": (sb - 1, per), "short_dst": (sb, per - 1)}[strides]
        yield "icamd_mip_pyramid_device", (comps, 256, 256, stride, 9, n, ss, ds, src, dst, N)

    def mip_codec_of(comp, fmt):
        if comp == 0 and fmt_comps(fmt):
            return 0 if fmt_comps(fmt) == 3 else 1
        return 2 if comp == 1 and fmt == 0 else -1
    for comp, fmt, (h, w), long_out in itertools.product([-1, 0, 1, 2], [-1, 0, 1, 2, 3], [(0, 8), (1, 1), (8, 8), (64, 64),
                                                                                          (12, 20), (65536, 65536)], [0, 1]):
        for levels in levels_of(h, w):
            out = C.icamd_mip_chain_size(mip_codec_of(comp, fmt), h, w, levels, None) + long_out
            yield "icamd_compress_mips", (comp, 2, fmt, h, w, 0, levels, A, A, out)
    for comp, pad, (src, dst) in itertools.product([0, 1], [4, 0xffffffff], [(A, A), (N, A), (A, N)]):
        yield "icamd_compress_mips", (comp, 2, 0, 8, 8, pad, 4, src, dst, C.icamd_mip_chain_size(mip_codec_of(comp, 0), 8, 8, 4,
                                                                                                 None))

    # ---- diagnostics
    for ptr, us in itertools.product([N, A, M4, M8], [0, 10000000, 10000001]):
        yield "icamd_clock_probe_device", (ptr, us, N)
    yield "icamd_wall_clock_rate_khz", ()
    yield "icamd_device_count", ()


# one character per status record: index into the outcome table
ALPHABET = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ!#$%&()*+,-./:;<=>?@[]^_{|}~"


def record(lib):
    """{entry: results} in grid order: sizes as numbers; statuses as a string of outcome indices, an outcome being
    [status, index of the icamd_last_error() text or null]"""
    texts, outcomes, results, calls = [], [], {}, {}
    for name, args in grid(lib):
        lib.keep = []
        if callable(args):
            args = args(lib)
        value = getattr(lib, name)(*args)
        calls.setdefault(name, []).append(args)
        if name in SIZE_RESULTS:
            results.setdefault(name, []).append(value)
            continue
        text = None
        if value < 0:
            t = lib.icamd_last_error().decode()
            if t not in texts:
                texts.append(t)
            text = texts.index(t)
        if [value, text] not in outcomes:
            outcomes.append([value, text])
        results.setdefault(name, []).append(ALPHABET[outcomes.index([value, text])])
    lib.keep = []
    for name in results:
        if name not in SIZE_RESULTS:
            results[name] = "".join(results[name])
    return {"texts": texts, "outcomes": outcomes, "results": results}, calls


def dump(table):
    lines = ['{', ' "texts": %s,' % json.dumps(table["texts"]), ' "outcomes": %s,' % json.dumps(table["outcomes"]),
             ' "results": {']
    items = sorted(table["results"].items())
    for i, (name, res) in enumerate(items):
        lines.append('  %s: %s%s' % (json.dumps(name), json.dumps(res), "," if i + 1 < len(items) else ""))
    lines += [' }', '}']
    return "\n".join(lines) + "\n"


def decode(table, name, i):
    res = table["results"][name][i]
    if name in SIZE_RESULTS:
        return res
    status, text = table["outcomes"][ALPHABET.index(res)]
    return status, None if text is None else table["texts"][text]


def load_lib():
    sys.path.insert(0, os.path.dirname(HERE))
    import ic_amd_loader
    return Lib(ic_amd_loader.load_package())


def test_statuses_and_error_texts_match_the_recorded_table():
    lib = load_lib()
    if lib.icamd_device_count() > 0:
        pytest.skip("a HIP device is visible: this table's dummy device pointers would reach a kernel launch")
    with open(GOLDEN) as f:
        want = json.load(f)
    got, calls = record(lib)
    assert sorted(got["results"]) == sorted(want["results"]), "the grid's entry points changed"
    bad = []
    for name in sorted(got["results"]):
        n = len(want["results"][name])
        assert len(got["results"][name]) == n, "%s: %d calls in the grid, %d recorded" % (name, len(got["results"][name]), n)
        for i in range(n):
            g, w = decode(got, name, i), decode(want, name, i)
            if g != w:
                bad.append("%s%s: got %r, recorded %r" % (name, tuple(calls[name][i]), g, w))
    assert not bad, "%d calls differ from the recorded table, first ones:\n%s" % (len(bad), "\n".join(bad[:20]))


if __name__ == "__main__":
    lib = load_lib()
    if lib.icamd_device_count() > 0:
        sys.exit("a HIP device is visible: record the table on a machine without one")
    table, _ = record(lib)
    with open(GOLDEN, "w") as f:
        f.write(dump(table))
    print("%s: %d calls, %d outcomes, %d texts" % (GOLDEN, sum(len(r) for r in table["results"].values()),
                                                   len(table["outcomes"]), len(table["texts"])))
