"""CPU tier for the BC4 / BC5 (RGTC) extension (include/ic_amd.h, ICAMD_BC4).

* The block math of image-compression_amd/csrc/bc45_block.h, compiled for the host (tests/host_emul/bc45_emul.cc,
  -DICAMD_HOST_EMULATION), against the definition computed with the oracle's DXT5 (tests/bc45_oracle.py), and the packed-row
  encoder against encode_dxt5_alpha_block on random blocks.
* The C ABI's host-side surface: sizes, kernel names, the ICAMD_ERR_ARG cases, container framing.
* (ref) the definition pinned to the compiled reference itself.
* The new kernels compile without scratch."""
import ctypes
import importlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bc45_oracle as B
import ic_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
pkg = importlib.import_module("image-compression_amd")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bc45") / "libbc45_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC, "-o", so,
                           os.path.join(EMUL_DIR, "bc45_emul.cc")])
    L = ctypes.CDLL(so)
    L.bc45_emul_encode.restype = ctypes.c_int
    L.bc45_emul_encode.argtypes = [T.ci, T.ci, T.ci, T.ci, T.u32, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp]
    L.bc45_emul_decode.restype = ctypes.c_int
    L.bc45_emul_decode.argtypes = [T.ci, T.u32, T.u32, T.u32, T.vp, T.vp]
    L.bc45_emul_block_both.restype = None
    L.bc45_emul_block_both.argtypes = [T.vp, T.ci, T.vp, T.vp]
    yield L
    T.assert_no_emul_violations(L, "test_bc45_host")


def emul_encode(L, codec, flat, h, w, comps, swap=0, gh=None, gw=None, stride=None, packed_only=0):
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    stride = w * comps if stride is None else stride
    out = np.zeros(B.encoded_size(codec, gh, gw), np.uint8)
    src = np.ascontiguousarray(flat, dtype=np.uint8).reshape(-1)
    assert L.bc45_emul_encode(codec, comps, swap, packed_only, h, w, gh, gw, stride, src.ctypes.data, out.ctypes.data)
    return out.tobytes()


def emul_decode(L, codec, blocks, h, w, pad=0):
    out = np.zeros(h * (w * B.comps_out(codec) + pad), np.uint8)
    b = np.frombuffer(bytes(blocks), np.uint8).copy()
    assert L.bc45_emul_decode(codec, h, w, pad, b.ctypes.data, out.ctypes.data)
    return out


@pytest.mark.parametrize("gen", sorted(B.GENERATORS))
def test_encoder_matches_definition_on_every_shape_and_layout(emul, gen):
    for i, (h, w, pad) in enumerate(B.SHAPES):
        img = B.image(gen, h, w, 4, index=i)
        for codec, comps, swap in B.LAYOUTS:
            src = np.ascontiguousarray(img[..., :comps])
            want = B.oracle_encode(codec, src, h, w, comps, swap)
            flat = T.with_row_padding(src, pad)
            for packed_only in (0, 1):
                got = emul_encode(emul, codec, flat, h, w, comps, swap, stride=w * comps + pad, packed_only=packed_only)
                assert got == want, (gen, h, w, pad, codec, comps, swap, packed_only)


@pytest.mark.parametrize("h,w,gh,gw", [(30, 30, 40, 48), (5, 3, 16, 16), (1, 1, 9, 13), (64, 61, 64, 64), (17, 33, 24, 48)])
def test_encoder_padded_grid_reaches_the_one_pixel_rule(emul, h, w, gh, gw):
    for gen in ("noise", "saturated"):
        img = B.image(gen, h, w, 4, index=h + w)
        for codec, comps, swap in B.LAYOUTS:
            src = np.ascontiguousarray(img[..., :comps])
            want = B.oracle_encode(codec, src, h, w, comps, swap, gh=gh, gw=gw)
            for packed_only in (0, 1):
                got = emul_encode(emul, codec, src, h, w, comps, swap, gh=gh, gw=gw, packed_only=packed_only)
                assert got == want, (gen, h, w, gh, gw, codec, comps, swap, packed_only)


def test_encoder_every_endpoint_distance_in_both_modes(emul):
    strip = B.every_range_strip()
    h, w = strip.shape
    rg = np.ascontiguousarray(np.stack([strip, strip[:, ::-1]], axis=-1))
    assert emul_encode(emul, B.BC4, strip, h, w, 1) == B.oracle_encode(B.BC4, strip, h, w, 1)
    assert emul_encode(emul, B.BC5, rg, h, w, 2) == B.oracle_encode(B.BC5, rg, h, w, 2)


def test_packed_rows_form_equals_the_dxt5_alpha_block(emul):
    g = np.random.Generator(np.random.PCG64(4242))
    a, b = np.zeros(8, np.uint8), np.zeros(8, np.uint8)
    for i in range(20000):
        kind = i % 4
        if kind == 0:
            v = g.integers(0, 256, 16)
        elif kind == 1:
            lo = int(g.integers(0, 256))
            v = np.clip(lo + g.integers(-4, 5, 16), 0, 255)
        elif kind == 2:
            v = g.choice(np.array([0, 1, 2, 127, 253, 254, 255]), 16)
        else:
            v = np.where(g.integers(0, 2, 16) == 1, g.integers(0, 256), g.integers(0, 256, 16))
        v = np.ascontiguousarray(v, np.uint8)
        emul.bc45_emul_block_both(v.ctypes.data, int(i % 97 == 0), a.ctypes.data, b.ctypes.data)
        assert a.tobytes() == b.tobytes(), v


@pytest.mark.parametrize("codec", [B.BC4, B.BC5])
def test_decoder_matches_definition(emul, codec):
    for i, (h, w, pad) in enumerate(B.SHAPES):
        words = B.random_words(codec, h, w, seed=100 + i)
        assert emul_decode(emul, codec, words, h, w, pad).tobytes() == B.oracle_decode(codec, words, h, w, pad).tobytes(), (h, w)
        img = B.image("mixed", h, w, 2, index=i)
        blocks = B.oracle_encode(codec, img[..., :B.comps_out(codec)], h, w, B.comps_out(codec))
        assert emul_decode(emul, codec, blocks, h, w, pad).tobytes() == B.oracle_decode(codec, blocks, h, w, pad).tobytes()


# ---- the C ABI's host-side surface (no device work: every check below returns before the GPU is touched)

def test_encoded_size_and_kernel_names():
    assert pkg.BC4 == 5 and pkg.BC5 == 6
    assert pkg.encoded_size(pkg.BC5, 8, 8) == 64 and pkg.encoded_size(pkg.BC4, 8, 8) == 32
    assert pkg.encoded_size(pkg.BC4, 5, 3) == 16 and pkg.encoded_size(pkg.BC5, 257, 1023) == 65 * 256 * 16
    assert pkg.encoded_size(pkg.DXT5, 8, 8) == 64 and pkg.encoded_size(pkg.DXT1, 8, 8) == 32  # unchanged
    names = {(5, 1): "icamd_bc4_r8_kernel", (5, 2): "icamd_bc4_rg8_kernel", (5, 3): "icamd_bc4_rgb888_kernel",
             (5, 4): "icamd_bc4_rgba8_kernel", (6, 2): "icamd_bc5_rg8_kernel", (6, 3): "icamd_bc5_rgb888_kernel",
             (6, 4): "icamd_bc5_rgba8_kernel"}
    for (codec, comps), name in names.items():
        assert pkg.kernel_name(codec, comps) == name
    assert pkg.kernel_name(pkg.BC5, 1) == ""


@pytest.mark.parametrize("codec,comps,swap", [(5, 0, 0), (5, 5, 0), (5, 1, 1), (5, 2, 1), (6, 1, 0), (6, 5, 0), (6, 2, 1)])
def test_encode_argument_errors(codec, comps, swap):
    lib = pkg.lib()
    dummy = ctypes.c_void_p(16)  # never dereferenced: the arguments are refused first
    st = lib.icamd_encode_device(codec, 0, comps, swap, 8, 8, 8, 8, 8 * max(comps, 1), 1, 0, 0, dummy, dummy, None)
    assert st == -4


def test_decode_swap_is_an_argument_error():
    lib = pkg.lib()
    dummy = ctypes.c_void_p(16)
    for codec in (pkg.BC4, pkg.BC5):
        assert lib.icamd_decode_device(codec, 1, 8, 8, 0, 1, 0, 0, dummy, dummy, None) == -4


def _level_bytes(codec, h, w, l):
    lh, lw = max(1, h >> l), max(1, w >> l)
    return ((lh + 3) // 4) * ((lw + 3) // 4) * (16 if codec == B.BC5 else 8)


def _levels(codec, h, w, n):
    g = np.random.default_rng(codec * 31 + n)
    return [g.integers(0, 256, _level_bytes(codec, h, w, l), dtype=np.uint8).tobytes() for l in range(n)]


def _dds(codec, h, w, levels):
    n = len(levels)
    flags = 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000 | (0x20000 if n > 1 else 0)
    caps = 0x1000 | ((0x8 | 0x400000) if n > 1 else 0)
    pf = struct.pack("<II4sIIIII", 32, 0x4, b"ATI1" if codec == B.BC4 else b"ATI2", 0, 0, 0, 0, 0)
    return b"DDS " + struct.pack("<IIIIIII", 124, flags, h, w, len(levels[0]), 0, n) + b"\0" * 44 + pf + \
        struct.pack("<IIIII", caps, 0, 0, 0, 0) + b"".join(levels)


def _ktx(codec, h, w, levels):
    internal, base = (0x8DBB, 0x1903) if codec == B.BC4 else (0x8DBD, 0x8227)  # COMPRESSED_RED_RGTC1 / RG_RGTC2, GL_RED / GL_RG
    return bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A]) + \
        struct.pack("<13I", 0x04030201, 0, 1, 0, internal, base, w, h, 0, 0, 1, len(levels), 0) + \
        b"".join(struct.pack("<I", len(b)) + b for b in levels)


def _pvr(codec, h, w, levels):
    return struct.pack("<IIQIIIIIIIII", 0x03525650, 0, 12 if codec == B.BC4 else 13, 0, 0, h, w, 1, 1, 1, len(levels), 0) + \
        b"".join(levels)


@pytest.mark.parametrize("codec", [B.BC4, B.BC5])
@pytest.mark.parametrize("h,w,n", [(64, 64, 1), (64, 64, 7), (61, 59, 3), (5, 3, 1), (256, 128, 9)])
def test_container_bytes(codec, h, w, n):
    levels = _levels(codec, h, w, n)
    for container, want in [(pkg.CONTAINER_DDS, _dds(codec, h, w, levels)), (pkg.CONTAINER_KTX, _ktx(codec, h, w, levels)),
                            (pkg.CONTAINER_PVR, _pvr(codec, h, w, levels))]:
        assert pkg.container_size(container, codec, h, w, n) == len(want)
        assert pkg.container_write(container, codec, h, w, levels) == want, (container, codec, h, w, n)


def test_container_pkm_and_pvrtc4_stay_refused():
    for codec in (pkg.BC4, pkg.BC5):
        assert pkg.container_size(pkg.CONTAINER_PKM, codec, 64, 64, 1) == 0
    lib = pkg.lib()
    out = (ctypes.c_uint8 * 256)()
    data = (ctypes.c_char_p * 1)(b"\0" * 8)
    sizes = (ctypes.c_size_t * 1)(8)
    assert lib.icamd_container_write(pkg.CONTAINER_DDS, 4, 4, 4, 1, data, sizes, out, 136) == -4
    assert lib.icamd_container_write(pkg.CONTAINER_KTX, 7, 4, 4, 1, data, sizes, out, 76) == -4


# ---- the definition against the compiled reference (build container only)

@pytest.mark.ref
@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("h,w", [(64, 64), (61, 59), (5, 3), (1, 1), (9, 2), (37, 130)])
def test_definition_against_the_reference(emul, h, w):
    for gen in ("mixed", "saturated"):
        img = B.image(gen, h, w, 2, index=h * w)
        for c in (0, 1):
            rgba = np.zeros((h, w, 4), np.uint8)
            rgba[..., 3] = img[..., c]
            ref = np.frombuffer(T.ref_compress(T.DXTC, T.RGBA, rgba, h, w), np.uint8).reshape(-1, 16)[:, :8].tobytes()
            chan = np.ascontiguousarray(img[..., c])
            assert emul_encode(emul, B.BC4, chan, h, w, 1) == ref, (gen, h, w, c)


# ---- build check: the new kernels keep everything in registers

def test_bc45_kernels_use_no_scratch(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path), "k.s")
    subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(T.ROOT, "include"),
                           "-I" + CSRC, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "bc45_kernels.hip")],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    import re
    metas = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        metas[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
    names = ["icamd_bc4_r8_kernel", "icamd_bc4_rg8_kernel", "icamd_bc4_rgb888_kernel", "icamd_bc4_rgba8_kernel",
             "icamd_bc5_rg8_kernel", "icamd_bc5_rgb888_kernel", "icamd_bc5_rgba8_kernel", "icamd_bc4_decode_kernel",
             "icamd_bc5_decode_kernel"]
    for n in names:
        assert n in metas, n
        assert metas[n] == 0, "%s uses %d bytes of scratch" % (n, metas[n])
