"""CPU tier for the ETC2 RGBA8 extension (include/ic_amd.h, ICAMD_ETC2_RGBA8).

* The block math of image-compression_amd/csrc/etc2_block.h fused with the ETC1 colour half, compiled for the host
  (tests/host_emul/etc2_emul.cc, -DICAMD_HOST_EMULATION), bit-exact against the numpy definition (tests/etc2_oracle.py).
* The table self-checks and the three derived quality conditions of the definition (blocks that use both extreme indices,
  flat blocks, 0 / 255 blocks: all decode exactly).
* The C ABI's host-side surface: sizes, kernel names, the ICAMD_ERR_ARG / ICAMD_FALSE cases, container framing.
* (ref) the colour half pinned to the compiled reference itself.
* The new kernels compile without scratch."""
import ctypes
import importlib
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bc45_oracle as B
import etc2_oracle as E
import ic_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
pkg = importlib.import_module("image-compression_amd")
PADDED = [(30, 30, 40, 48), (5, 3, 16, 16), (1, 1, 9, 13), (64, 61, 64, 64), (17, 33, 24, 48)]


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("etc2") / "libetc2_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC,
                           "-I" + os.path.join(T.ROOT, "include"), "-o", so, os.path.join(EMUL_DIR, "etc2_emul.cc")])
    L = ctypes.CDLL(so)
    L.etc2_emul_encode.restype = ctypes.c_int
    L.etc2_emul_encode.argtypes = [T.ci, T.u32, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp]
    L.etc2_emul_decode.restype = ctypes.c_int
    L.etc2_emul_decode.argtypes = [T.ci, T.u32, T.u32, T.u32, T.vp, T.vp]
    L.etc2_emul_alpha_block.restype = None
    L.etc2_emul_alpha_block.argtypes = [T.vp, T.vp, T.vp]
    L.etc2_emul_modifier.restype = ctypes.c_int
    L.etc2_emul_modifier.argtypes = [T.ci, T.ci]
    yield L
    T.assert_no_emul_violations(L, "test_etc2_host")


def emul_encode(L, flat, h, w, strategy, gh=None, gw=None, stride=None):
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    out = np.zeros(E.encoded_size(gh, gw), np.uint8)
    src = np.ascontiguousarray(flat, dtype=np.uint8).reshape(-1)
    assert L.etc2_emul_encode(strategy, h, w, gh, gw, w * 4 if stride is None else stride, src.ctypes.data, out.ctypes.data)
    return out.tobytes()


def emul_decode(L, blocks, h, w, swap=0, pad=0):
    out = np.zeros(h * (w * 4 + pad), np.uint8)
    b = np.frombuffer(bytes(blocks), np.uint8).copy()
    assert L.etc2_emul_decode(swap, h, w, pad, b.ctypes.data, out.ctypes.data)
    return out


def emul_alpha_words(L, blocks16):
    """[n, 16] alphas in RASTER order -> ([n, 8] words, [n, 16] decoded alphas in raster order)."""
    v = np.ascontiguousarray(blocks16, np.uint8)
    words, dec = np.zeros((v.shape[0], 8), np.uint8), np.zeros((v.shape[0], 16), np.uint8)
    for i in range(v.shape[0]):
        L.etc2_emul_alpha_block(v[i].ctypes.data, words[i].ctypes.data, dec[i].ctypes.data)
    return words, dec


def raster_to_texel(v):
    """[n, 16] raster order (4 y + x) -> the definition's texel order (4 x + y)."""
    return np.asarray(v).reshape(-1, 4, 4).transpose(0, 2, 1).reshape(-1, 16)


# ---- the modifier table

def test_table_self_checks(emul):
    got = np.array([[emul.etc2_emul_modifier(t, k) for k in range(8)] for t in range(16)])
    assert (got == E.M).all()
    for M in (got, E.M):
        assert (M[:, 4:] == -M[:, :4] - 1).all()
        assert M.sum() == -64
        assert (M[:, 7] - M[:, 3]).tolist() == [29, 25, 25, 25, 23, 21, 21, 21, 19, 19, 19, 19, 19, 19, 17, 17]


# ---- encoder against the definition

@pytest.mark.parametrize("gen", sorted(B.GENERATORS))
def test_encoder_matches_definition_on_every_shape_and_layout(emul, gen):
    for i, (h, w, pad) in enumerate(B.SHAPES):
        img = B.image(gen, h, w, 4, index=i)
        flat = T.with_row_padding(img, pad)
        alpha = E.eac_encode(E.block_alphas(img[..., 3], h, w, h, w))
        largest = h * w == max(s[0] * s[1] for s in B.SHAPES)
        for strategy in ((T.SMALLER_ERROR,) if largest else E.STRATEGIES):
            got = emul_encode(emul, flat, h, w, strategy, stride=w * 4 + pad)  # (swap_rb never reaches the block math)
            for swap in (0, 1):
                want = E.oracle_encode(img, h, w, swap, strategy, alpha_words=alpha)
                assert got == want, (gen, h, w, pad, strategy, swap)


@pytest.mark.parametrize("h,w,gh,gw", PADDED)
def test_encoder_padded_grid(emul, h, w, gh, gw):
    for gen in ("noise", "saturated"):
        img = B.image(gen, h, w, 4, index=h + w)
        for strategy in E.STRATEGIES:
            want = E.oracle_encode(img, h, w, 0, strategy, gh=gh, gw=gw)
            assert emul_encode(emul, img, h, w, strategy, gh=gh, gw=gw) == want, (gen, h, w, gh, gw, strategy)


def test_encoder_every_range(emul):
    strip = E.every_range_strip()
    h, w = strip.shape
    img = B.image("noise", h, w, 4, index=77)
    img[..., 3] = strip
    assert emul_encode(emul, img, h, w, T.HEURISTIC) == E.oracle_encode(img, h, w, 0, T.HEURISTIC)


# ---- the derived quality conditions, on the library's own output decoded by the library's own decoder

def test_blocks_that_use_both_extreme_indices_are_reproduced(emul):
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9200))
    blocks = []
    while len(blocks) < 300:
        t, m = int(g.integers(0, 16)), int(g.integers(1, 16))
        lo_b, hi_b = -int(E.M[t, 3]) * m, 255 - int(E.M[t, 7]) * m  # bases for which neither extreme clamps
        if lo_b > hi_b:
            continue
        b = int(g.integers(lo_b, hi_b + 1))
        idx = g.integers(0, 8, 16)
        idx[g.permutation(16)[:2]] = (3, 7)
        blocks.append(b + E.M[t, idx] * m)
    v = np.array(blocks)
    assert v.min() >= 0 and v.max() <= 255
    words, dec = emul_alpha_words(emul, v)
    assert (dec == v).all()
    assert (words == E.eac_encode(raster_to_texel(v))).all()


def test_flat_blocks_of_every_value_decode_exactly(emul):
    v = np.repeat(np.arange(256)[:, None], 16, axis=1)
    words, dec = emul_alpha_words(emul, v)
    assert (dec == v).all()
    assert (words == E.eac_encode(v)).all()
    assert ((words[:, 1] >> 4) != 0).all()  # multiplier 0 is never written


def test_blocks_of_0_and_255_decode_exactly(emul):
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9300))
    v = g.integers(0, 2, size=(300, 16)) * 255
    v[0], v[1], v[2, 0], v[3, 15] = 0, 255, 255, 0
    words, dec = emul_alpha_words(emul, v)
    assert (dec == v).all()
    assert (words == E.eac_encode(raster_to_texel(v))).all()


# ---- decoder

def test_decoder_matches_definition(emul):
    for i, (h, w, pad) in enumerate(B.SHAPES[:-1]):
        words = E.random_words(h, w, seed=300 + i)
        al = np.frombuffer(words, np.uint8).reshape(-1, 16)
        if al.shape[0] >= 8:
            assert ((al[:, 1] >> 4) == 0).any() and (al[:, 0] == 0).any() and (al[:, 0] == 255).any()
        for swap in (0, 1):
            assert emul_decode(emul, words, h, w, swap, pad).tobytes() == E.oracle_decode(words, h, w, swap, pad).tobytes(), (h, w, swap)
        img = B.image("mixed", h, w, 4, index=i)
        blocks = E.oracle_encode(img, h, w)
        assert emul_decode(emul, blocks, h, w, 0, pad).tobytes() == E.oracle_decode(blocks, h, w, 0, pad).tobytes()


def test_multiplier_zero_decodes_to_base():
    words = np.zeros((4, 8), np.uint8)
    words[:, 0] = (0, 7, 200, 255)
    words[:, 1] = (0x00, 0x05, 0x0d, 0x0f)
    words[:, 2:] = 0xb6
    assert (E.eac_decode(words) == words[:, :1].astype(np.int64)).all()


# ---- the C ABI's host-side surface (no device work: every check below returns before the GPU is touched)

def test_codec_value_sizes_and_kernel_names():
    assert pkg.ETC2_RGBA8 == 16 == E.ETC2_RGBA8
    assert pkg.encoded_size(pkg.ETC2_RGBA8, 8, 8) == 64 and pkg.encoded_size(pkg.ETC2_RGBA8, 5, 3) == 32
    assert pkg.encoded_size(pkg.ETC2_RGBA8, 257, 1023) == 65 * 256 * 16
    assert pkg.encoded_size(pkg.ETC1, 8, 8) == 32  # unchanged
    assert pkg.kernel_name(pkg.ETC2_RGBA8, 4) == "icamd_etc2_rgba8_kernel"
    assert pkg.kernel_name(pkg.ETC2_RGBA8, 3) == ""
    assert pkg.metric_kernel_name(pkg.ETC2_RGBA8, 4) == "icamd_metric_etc2_rgba8_kernel"
    assert pkg.metric_kernel_name(pkg.ETC2_RGBA8, 3) == ""
    assert pkg.mip_chain_size(pkg.ETC2_RGBA8, 64, 64, 3) == (0, None) and pkg.mip_kernel_name(pkg.ETC2_RGBA8, 4) == ""


def test_compressor_format_mapping_is_unchanged():
    lib = pkg.lib()
    for fmt in (pkg.RGB, pkg.BGR, pkg.RGBA, pkg.BGRA):
        assert lib.icamd_supports_format(pkg.COMPRESSOR_ETC, fmt) == (1 if fmt == pkg.RGB else 0)
    assert pkg.compute_compressed_data_size(pkg.COMPRESSOR_ETC, pkg.RGBA, 8, 8) == 0


def test_argument_errors():
    lib = pkg.lib()
    dummy = ctypes.c_void_p(16)  # never dereferenced: the arguments are refused first
    for comps in (0, 1, 2, 3, 5):
        assert lib.icamd_encode_device(16, 2, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, dummy, dummy, None) == -4, comps
        assert lib.icamd_measure_error_device(16, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, dummy, dummy, dummy, None) == -4, comps
    assert lib.icamd_encode_device(16, 2, 4, 0, 0, 8, 8, 8, 32, 1, 0, 0, dummy, dummy, None) == 1    # empty image
    assert lib.icamd_encode_device(16, 2, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, None, dummy, None) == 1     # null source
    assert lib.icamd_decode_device(16, 0, 8, 0, 0, 1, 0, 0, dummy, dummy, None) == 1
    assert lib.icamd_measure_error_device(16, 4, 0, 8, 8, 8, 8, 31, 1, 0, 0, dummy, dummy, dummy, None) == -4  # stride < row
    assert lib.icamd_measure_error_device(16, 4, 0, 8, 8, 4, 8, 32, 1, 0, 0, dummy, dummy, dummy, None) == -4  # grid < image
    assert lib.icamd_encode_mips_device(16, 2, 4, 0, 8, 8, 32, 1, 1, 0, 0, dummy, dummy, None, 0, None) == -4  # as for PVRTC
    assert lib.icamd_encode_mips_device(pkg.PVRTC2, 2, 4, 0, 8, 8, 32, 1, 1, 0, 0, dummy, dummy, None, 0, None) == -4


@pytest.mark.parametrize("codec", list(range(7, 16)) + [17])
def test_unassigned_codec_values_are_rejected(codec):
    lib = pkg.lib()
    dummy = ctypes.c_void_p(16)
    assert pkg.kernel_name(codec, 4) == "" and pkg.metric_kernel_name(codec, 4) == ""
    assert lib.icamd_decode_device(codec, 0, 8, 8, 0, 1, 0, 0, dummy, dummy, None) == 1
    assert lib.icamd_measure_error_device(codec, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, dummy, dummy, dummy, None) == -4
    for container in (pkg.CONTAINER_DDS, pkg.CONTAINER_KTX, pkg.CONTAINER_PKM, pkg.CONTAINER_PVR):
        assert pkg.container_size(container, codec, 8, 8, 1) == 0
    out = (ctypes.c_uint8 * 256)()
    data = (ctypes.c_char_p * 1)(b"\0" * 16)
    sizes = (ctypes.c_size_t * 1)(16)
    assert lib.icamd_container_write(pkg.CONTAINER_KTX, codec, 4, 4, 1, data, sizes, out, 84) == -4


def _levels(h, w, n):
    g = np.random.default_rng(160 + n)
    return [g.integers(0, 256, ((max(1, h >> l) + 3) // 4) * ((max(1, w >> l) + 3) // 4) * 16, dtype=np.uint8).tobytes()
            for l in range(n)]


def _ktx(h, w, levels):
    return bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A]) + \
        struct.pack("<13I", 0x04030201, 0, 1, 0, 0x9278, 0x1908, w, h, 0, 0, 1, len(levels), 0) + \
        b"".join(struct.pack("<I", len(b)) + b for b in levels)


def _pvr(h, w, levels):
    return struct.pack("<IIQIIIIIIIII", 0x03525650, 0, 23, 0, 0, h, w, 1, 1, 1, len(levels), 0) + b"".join(levels)


def _pkm(h, w, levels):
    return b"PKM 20" + struct.pack(">HHHHH", 3, (w + 3) & ~3, (h + 3) & ~3, w, h) + levels[0]


@pytest.mark.parametrize("h,w,n", [(64, 64, 1), (64, 64, 7), (61, 59, 3), (5, 3, 1), (256, 128, 9)])
def test_container_bytes(h, w, n):
    levels = _levels(h, w, n)
    cases = [(pkg.CONTAINER_KTX, _ktx(h, w, levels)), (pkg.CONTAINER_PVR, _pvr(h, w, levels))]
    if n == 1:
        cases.append((pkg.CONTAINER_PKM, _pkm(h, w, levels)))
    for container, want in cases:
        assert pkg.container_size(container, 16, h, w, n) == len(want)
        assert pkg.container_write(container, 16, h, w, levels) == want, (container, h, w, n)
    assert pkg.container_size(pkg.CONTAINER_DDS, 16, h, w, n) == pkg.container_size(pkg.CONTAINER_DDS, pkg.ETC1, h, w, n) == 0
    if n > 1:
        assert pkg.container_size(pkg.CONTAINER_PKM, 16, h, w, n) == 0


def test_etc1_pkm_header_is_unchanged():
    data = b"\x11" * 8
    assert pkg.container_write(pkg.CONTAINER_PKM, pkg.ETC1, 4, 4, [data])[:8] == b"PKM 10\0\0"


# ---- the colour half against the compiled reference (build container only)

@pytest.mark.ref
@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("h,w", [(64, 64), (61, 59), (5, 3), (1, 1), (9, 2), (37, 130)])
def test_colour_half_against_the_reference(emul, h, w):
    for gen in ("mixed", "saturated"):
        img = B.image(gen, h, w, 4, index=h * w)
        rgb = np.ascontiguousarray(img[..., :3])
        for strategy in E.STRATEGIES:
            ref = T.ref_compress(T.ETC, T.RGB, rgb, h, w, strategy=strategy)
            got = np.frombuffer(emul_encode(emul, img, h, w, strategy), np.uint8).reshape(-1, 16)[:, 8:].tobytes()
            assert got == ref, (gen, h, w, strategy)


# ---- build check: the new kernels keep everything in registers

def test_etc2_kernels_use_no_scratch(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    metas = {}
    for unit in ("etc2_kernels.hip", "metric_kernels.hip"):
        out = os.path.join(str(tmp_path), unit + ".s")
        subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(T.ROOT, "include"),
                               "-I" + CSRC, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, unit)],
                              stderr=subprocess.DEVNULL)
        for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", open(out).read(), re.S):
            blk = m.group(0)
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            metas[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
    names = ["icamd_etc2_rgba8_kernel", "icamd_etc2_rgba8_split_h_kernel", "icamd_etc2_rgba8_split_v_kernel",
             "icamd_etc2_rgba8_heuristic_kernel", "icamd_etc2_rgba8_decode_kernel", "icamd_metric_etc2_rgba8_kernel"]
    for n in names:
        assert n in metas, n
        assert metas[n] == 0, "%s uses %d bytes of scratch" % (n, metas[n])
