"""CPU tier for the complete ETC2 colour word and ICAMD_ETC2_RGB8 (include/ic_amd.h).

* The block math of image-compression_amd/csrc/etc2_colour_block.h compiled for the host
  (tests/host_emul/etc2_colour_emul.cc, -DICAMD_HOST_EMULATION), bit-exact against the numpy definition
  (tests/etc2_colour_oracle.py): five-mode decode, planar fit / pack, the ETC1-or-planar choice.
* Four known answers of the decoder, as literals, through both.
* The C ABI's host-side surface of codec 18: sizes, kernel names, container headers, the ICAMD_ERR_ARG cases.
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
import etc2_colour_oracle as C
import etc2_oracle as E
import ic_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
pkg = importlib.import_module("image-compression_amd")
PADDED = [(30, 30, 40, 48), (5, 3, 16, 16), (1, 1, 9, 13), (64, 61, 64, 64), (17, 33, 24, 48)]  # as test_etc2_host.py

# 16 RGB texels in raster order (4 y + x), computed by a separate script from the rules of DESIGN.md 3.13
KNOWN = {
    "045ac37e1b2de487": (C.T_MODE, [
        (163, 10, 78), (0, 85, 170), (204, 51, 119), (204, 51, 119), (245, 92, 160), (204, 51, 119), (204, 51, 119), (245, 92, 160),
        (163, 10, 78), (0, 85, 170), (245, 92, 160), (245, 92, 160), (204, 51, 119), (245, 92, 160), (204, 51, 119), (245, 92, 160)]),
    "7bfb69d61b2de487": (C.H_MODE, [  # C1 >= C2
        (189, 19, 138), (255, 151, 255), (253, 83, 202), (253, 83, 202), (223, 87, 206), (253, 83, 202), (253, 83, 202), (223, 87, 206),
        (189, 19, 138), (255, 151, 255), (223, 87, 206), (223, 87, 206), (253, 83, 202), (223, 87, 206), (253, 83, 202), (223, 87, 206)]),
    "1104e9d31b2de487": (C.H_MODE, [  # C1 < C2
        (210, 40, 159), (45, 45, 28), (232, 62, 181), (232, 62, 181), (23, 23, 6), (232, 62, 181), (232, 62, 181), (23, 23, 6),
        (210, 40, 159), (45, 45, 28), (23, 23, 6), (23, 23, 6), (232, 62, 181), (23, 23, 6), (232, 62, 181), (23, 23, 6)]),
    "954806fa29087fff": (C.PLANAR, [  # O = (10, 100, 5), H = (60, 20, 33), V = (3, 127, 63) as codes
        (40, 201, 20), (91, 161, 49), (142, 121, 77), (192, 80, 106), (33, 215, 79), (84, 174, 107), (135, 134, 136), (185, 94, 164),
        (26, 228, 138), (77, 188, 166), (128, 148, 195), (178, 107, 223), (19, 242, 196), (70, 201, 225), (121, 161, 253), (171, 121, 255)]),
}


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("etc2c") / "libetc2_colour_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC,
                           "-I" + os.path.join(T.ROOT, "include"), "-o", so, os.path.join(EMUL_DIR, "etc2_colour_emul.cc")])
    L = ctypes.CDLL(so)
    L.etc2c_emul_encode.restype = ctypes.c_int
    L.etc2c_emul_encode.argtypes = [T.ci, T.ci, T.u32, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp]
    for fn in (L.etc2c_emul_decode_words, L.etc2c_emul_modes, L.etc2c_emul_planar_fit):
        fn.restype = None
        fn.argtypes = [T.u32, T.vp, T.vp]
    L.etc2c_emul_planar_pack.restype = None
    L.etc2c_emul_planar_pack.argtypes = [T.u32, T.vp, T.vp, T.vp]
    L.etc2c_emul_decode_rgba8.restype = ctypes.c_int
    L.etc2c_emul_decode_rgba8.argtypes = [T.ci, T.u32, T.u32, T.u32, T.vp, T.vp]
    yield L
    T.assert_no_emul_violations(L, "test_etc2_colour_host")


def emul_decode_words(L, words):
    b = np.frombuffer(bytes(words), np.uint8).copy()
    out = np.zeros((b.size // 8, 4, 4, 3), np.uint8)
    L.etc2c_emul_decode_words(b.size // 8, b.ctypes.data, out.ctypes.data)
    return out


def emul_encode(L, flat, h, w, comps, strategy, gh=None, gw=None, stride=None):
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    out = np.zeros(C.encoded_size(gh, gw), np.uint8)
    src = np.ascontiguousarray(flat, dtype=np.uint8).reshape(-1)
    assert L.etc2c_emul_encode(strategy, comps, h, w, gh, gw, w * comps if stride is None else stride, src.ctypes.data, out.ctypes.data)
    return out.tobytes()


# ---- decoder

@pytest.mark.parametrize("word", sorted(KNOWN))
def test_known_answers(emul, word):
    mode, texels = KNOWN[word]
    b = bytes.fromhex(word)
    want = np.array(texels, np.uint8).reshape(1, 4, 4, 3)
    assert C.modes(b).tolist() == [mode]
    assert (C.decode_blocks(b) == want).all()
    assert (emul_decode_words(emul, b) == want).all()


@pytest.mark.parametrize("mode", [C.INDIVIDUAL, C.DIFFERENTIAL, C.T_MODE, C.H_MODE, C.PLANAR])
def test_decoder_matches_definition_on_every_mode(emul, mode):
    n = 1 << 16
    words = C.random_colour_words(4, 4 * n, seed=700 + mode, only=mode)
    assert (C.modes(words) == mode).all()
    got_modes = np.zeros(n, np.uint8)
    b = np.frombuffer(words, np.uint8).copy()
    emul.etc2c_emul_modes(n, b.ctypes.data, got_modes.ctypes.data)
    assert (got_modes == {C.INDIVIDUAL: 0, C.DIFFERENTIAL: 0, C.T_MODE: 1, C.H_MODE: 2, C.PLANAR: 3}[mode]).all()
    assert (emul_decode_words(emul, words) == C.decode_blocks(words)).all()


def test_random_colour_words_interleave_the_five_modes():
    m = C.modes(C.random_colour_words(4, 1024, seed=11))
    assert (m == np.arange(256) % 5).all()


def test_etc2_rgba8_decodes_all_five_modes(emul):
    for i, (h, w, pad) in enumerate([(4, 1024, 0), (5, 3, 0), (17, 33, 5)]):
        words = np.frombuffer(E.random_words(h, w, seed=800 + i), np.uint8).reshape(-1, 16).copy()
        words[:, 8:] = np.frombuffer(C.random_colour_words(h, w, seed=810 + i), np.uint8).reshape(-1, 8)
        for swap in (0, 1):
            out = np.zeros(h * (w * 4 + pad), np.uint8)
            assert emul.etc2c_emul_decode_rgba8(swap, h, w, pad, words.ctypes.data, out.ctypes.data)
            assert out.tobytes() == C.oracle_decode_rgba8(words.tobytes(), h, w, swap, pad).tobytes(), (h, w, swap)


def test_etc1_compatible_rgba8_words_decode_as_before(emul):
    # the pre-existing definition (etc2_oracle.oracle_decode: the ETC1 oracle's colour) on the words it covers
    for i, (h, w, pad) in enumerate(B.SHAPES[:-1]):
        words = E.random_words(h, w, seed=300 + i)
        b = np.frombuffer(words, np.uint8).copy()
        for swap in (0, 1):
            out = np.zeros(h * (w * 4 + pad), np.uint8)
            assert emul.etc2c_emul_decode_rgba8(swap, h, w, pad, b.ctypes.data, out.ctypes.data)
            assert out.tobytes() == E.oracle_decode(words, h, w, swap, pad).tobytes(), (h, w, swap)
            assert out.tobytes() == C.oracle_decode_rgba8(words, h, w, swap, pad).tobytes()


# ---- planar fit and pack

def _all_codes(seed, n):
    g = np.random.Generator(np.random.PCG64(T.SEED0 + seed))
    codes = np.stack([g.integers(0, 128 if i % 3 == 1 else 64, n) for i in range(9)], axis=1)
    codes[0, :] = 0
    codes[1, :] = [63, 127, 63] * 3
    return codes


def test_every_packed_planar_word_is_planar_and_round_trips(emul):
    # every origin (the three fields that share bytes 0..2 with the ignored bits), the other six fields random
    ro, go, bo = np.meshgrid(np.arange(64), np.arange(128), np.arange(64), indexing="ij")
    n = ro.size
    codes = _all_codes(9600, n)
    codes[:, 0], codes[:, 1], codes[:, 2] = ro.reshape(-1), go.reshape(-1), bo.reshape(-1)
    want = C.planar_pack(codes)
    assert (C.modes(want) == C.PLANAR).all()
    assert (C.planar_fields(want) == codes).all()
    c32 = np.ascontiguousarray(codes, np.uint32)
    words, fields = np.zeros((n, 8), np.uint8), np.zeros((n, 9), np.uint32)
    emul.etc2c_emul_planar_pack(n, c32.ctypes.data, words.ctypes.data, fields.ctypes.data)
    assert (words == want).all()
    assert (fields == c32).all()
    got_modes = np.zeros(n, np.uint8)
    emul.etc2c_emul_modes(n, words.ctypes.data, got_modes.ctypes.data)
    assert (got_modes == 3).all()
    assert (emul_decode_words(emul, words[::97]) == C.planar_texels(codes[::97])).all()


def test_planar_fit_matches_definition(emul):
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9610))
    n = 20000
    tex = g.integers(0, 256, (n, 4, 4, 3), dtype=np.uint8)
    y, x = np.mgrid[0:4, 0:4]
    # exact planes (clamped), extremes, and noise
    o, dx, dy = g.integers(0, 256, (n // 2, 1, 1, 3)), g.integers(-40, 41, (n // 2, 1, 1, 3)), g.integers(-40, 41, (n // 2, 1, 1, 3))
    tex[:n // 2] = np.clip(o + x[None, :, :, None] * dx + y[None, :, :, None] * dy, 0, 255)
    tex[0], tex[1] = 0, 255
    tex[2, :, :2], tex[2, :, 2:] = 0, 255   # the steepest ramps: numerators far outside 0..20400
    tex[3, :2], tex[3, 2:] = 255, 0
    codes = np.zeros((n, 9), np.uint32)
    flat = np.ascontiguousarray(tex.reshape(n, 48))
    emul.etc2c_emul_planar_fit(n, flat.ctypes.data, codes.ctypes.data)
    assert (codes == C.planar_fit(tex)).all()


def test_a_flat_block_at_a_code_value_is_reproduced():
    # derived condition: a flat block whose channels sit on expanded code values is its own least-squares plane, exactly
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9620))
    codes = np.stack([g.integers(8, 56, 500) if i % 3 != 1 else g.integers(16, 112, 500) for i in range(9)], axis=1)
    codes[:, 3:6] = codes[:, 0:3]  # H = O and V = O
    codes[:, 6:9] = codes[:, 0:3]
    tex = C.planar_texels(codes)
    assert (C.planar_texels(C.planar_fit(tex)) == tex).all()


# ---- encoder against the definition

@pytest.mark.parametrize("h,w,gh,gw", PADDED)
def test_encoder_padded_grid(emul, h, w, gh, gw):
    for comps in (3, 4):
        for gen in ("smooth", "mixed"):
            img = B.image(gen, h, w, comps, index=h + w)
            for strategy in C.STRATEGIES:
                want, planar = C.oracle_encode(img, h, w, comps, 0, strategy, gh=gh, gw=gw, return_choice=True)
                got = emul_encode(emul, img, h, w, comps, strategy, gh=gh, gw=gw)
                assert got == want, (gen, h, w, gh, gw, comps, strategy)
                etc1 = np.frombuffer(T.oracle_encode(T.ETC1, img, h, w, comps, 0, strategy, gh=max(gh, h), gw=max(gw, w)), np.uint8)
                g8, e8 = np.frombuffer(got, np.uint8).reshape(-1, 8), etc1.reshape(-1, 8)
                same = (g8 == e8).all(axis=1)
                assert (same == ~planar).all()
                assert (C.modes(g8[~same]) == C.PLANAR).all()  # every block is the ETC1 oracle's bytes or a planar word


def test_encoder_smooth_left_noise_right(emul):
    for comps in (3, 4):
        img = C.smooth_and_noise(comps)
        for strategy in C.STRATEGIES:
            want, planar = C.oracle_encode(img, 64, 64, comps, 0, strategy, return_choice=True)
            assert planar.sum() >= 64 and (~planar).sum() >= 64  # both outcomes in numbers, by the definition alone
            assert emul_encode(emul, img, 64, 64, comps, strategy) == want, (comps, strategy)
            etc1 = np.frombuffer(T.oracle_encode(T.ETC1, img, 64, 64, comps, 0, strategy), np.uint8).reshape(-1, 8)
            g8 = np.frombuffer(want, np.uint8).reshape(-1, 8)
            assert (g8[~planar] == etc1[~planar]).all() and (C.modes(g8[planar]) == C.PLANAR).all()


def test_encoder_row_padding_and_swap_do_not_enter(emul):
    h, w, pad = 13, 22, 5
    img = B.image("smooth", h, w, 3, index=3)
    flat = T.with_row_padding(img, pad)
    for swap in (0, 1):  # (swap_rb never reaches the block math: bytes 0..2 as they lie in memory)
        assert emul_encode(emul, flat, h, w, 3, 2, stride=w * 3 + pad) == C.oracle_encode(img, h, w, 3, swap, 2)


# ---- the C ABI's host-side surface (no device work: every check below returns before the GPU is touched)

def test_codec_value_sizes_and_kernel_names():
    assert pkg.ETC2_RGB8 == 18 == C.ETC2_RGB8
    assert pkg.encoded_size(18, 8, 8) == 32 and pkg.encoded_size(18, 5, 3) == 16
    assert pkg.encoded_size(18, 257, 1023) == 65 * 256 * 8
    assert pkg.kernel_name(18, 3) == "icamd_etc2_rgb8_rgb888_kernel"
    assert pkg.kernel_name(18, 4) == "icamd_etc2_rgb8_rgba8_kernel"
    assert pkg.kernel_name(18, 2) == "" and pkg.kernel_name(18, 5) == ""
    assert pkg.metric_kernel_name(18, 3) == "icamd_metric_etc2_rgb8_rgb888_kernel"
    assert pkg.metric_kernel_name(18, 4) == "icamd_metric_etc2_rgb8_rgba8_kernel"
    assert pkg.metric_kernel_name(18, 2) == ""
    assert pkg.mip_chain_size(18, 64, 64, 3) == (0, None) and pkg.mip_kernel_name(18, 3) == ""
    assert pkg.kernel_name(pkg.ETC2_RGBA8, 4) == "icamd_etc2_rgba8_kernel"  # unchanged


def test_argument_errors():
    lib = pkg.lib()
    dummy = ctypes.c_void_p(16)  # never dereferenced: the arguments are refused first
    for comps in (0, 1, 2, 5):
        assert lib.icamd_encode_device(18, 2, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, dummy, dummy, None) == -4, comps
        assert lib.icamd_measure_error_device(18, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, dummy, dummy, dummy, None) == -4, comps
    assert lib.icamd_encode_device(18, 2, 3, 0, 0, 8, 8, 8, 24, 1, 0, 0, dummy, dummy, None) == 1    # empty image
    assert lib.icamd_encode_device(18, 2, 3, 0, 8, 8, 8, 8, 24, 1, 0, 0, None, dummy, None) == 1     # null source
    assert lib.icamd_decode_device(18, 0, 8, 0, 0, 1, 0, 0, dummy, dummy, None) == 1
    assert lib.icamd_measure_error_device(18, 3, 0, 8, 8, 8, 8, 23, 1, 0, 0, dummy, dummy, dummy, None) == -4  # stride < row
    assert lib.icamd_measure_error_device(18, 3, 0, 8, 8, 4, 8, 24, 1, 0, 0, dummy, dummy, dummy, None) == -4  # grid < image
    for comps in (3, 4):  # the mip entry points, as for ETC2 RGBA8
        assert lib.icamd_encode_mips_device(18, 2, comps, 0, 8, 8, 8 * comps, 1, 1, 0, 0, dummy, dummy, None, 0, None) == -4
        assert lib.icamd_encode_mips_filtered_device(18, 2, comps, 0, 0, 8, 8, 8 * comps, 1, 1, 0, 0, dummy, dummy, None, 0, None) == -4
    assert pkg.lib().icamd_mip_workspace_size(18, 3, 64, 64, 3, 1) == 0


def test_17_is_still_unassigned():
    lib = pkg.lib()
    dummy = ctypes.c_void_p(16)
    assert pkg.kernel_name(17, 3) == "" and pkg.kernel_name(17, 4) == "" and pkg.metric_kernel_name(17, 3) == ""
    assert lib.icamd_decode_device(17, 0, 8, 8, 0, 1, 0, 0, dummy, dummy, None) == 1
    assert lib.icamd_measure_error_device(17, 3, 0, 8, 8, 8, 8, 24, 1, 0, 0, dummy, dummy, dummy, None) == -4
    for container in (pkg.CONTAINER_DDS, pkg.CONTAINER_KTX, pkg.CONTAINER_PKM, pkg.CONTAINER_PVR):
        assert pkg.container_size(container, 17, 8, 8, 1) == 0


def test_host_buffer_entry_points_do_not_reach_the_codec():
    lib = pkg.lib()
    for fmt in (pkg.RGB, pkg.BGR, pkg.RGBA, pkg.BGRA):
        assert lib.icamd_supports_format(pkg.COMPRESSOR_ETC, fmt) == (1 if fmt == pkg.RGB else 0)
    assert pkg.compute_compressed_data_size(pkg.COMPRESSOR_ETC, pkg.RGB, 8, 8) == 32


def _levels(h, w, n):
    g = np.random.default_rng(180 + n)
    return [g.integers(0, 256, ((max(1, h >> l) + 3) // 4) * ((max(1, w >> l) + 3) // 4) * 8, dtype=np.uint8).tobytes()
            for l in range(n)]


def _ktx(h, w, levels):
    return bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A]) + \
        struct.pack("<13I", 0x04030201, 0, 1, 0, 0x9274, 0x1907, w, h, 0, 0, 1, len(levels), 0) + \
        b"".join(struct.pack("<I", len(b)) + b for b in levels)


def _pvr(h, w, levels):
    return struct.pack("<IIQIIIIIIIII", 0x03525650, 0, 22, 0, 0, h, w, 1, 1, 1, len(levels), 0) + b"".join(levels)


def _pkm(h, w, levels):
    return b"PKM 20" + struct.pack(">HHHHH", 1, (w + 3) & ~3, (h + 3) & ~3, w, h) + levels[0]


@pytest.mark.parametrize("h,w,n", [(64, 64, 1), (64, 64, 7), (61, 59, 3), (5, 3, 1)])
def test_container_bytes(h, w, n):
    levels = _levels(h, w, n)
    cases = [(pkg.CONTAINER_KTX, _ktx(h, w, levels)), (pkg.CONTAINER_PVR, _pvr(h, w, levels))]
    if n == 1:
        cases.append((pkg.CONTAINER_PKM, _pkm(h, w, levels)))
    for container, want in cases:
        assert pkg.container_size(container, 18, h, w, n) == len(want)
        assert pkg.container_write(container, 18, h, w, levels) == want, (container, h, w, n)
    assert pkg.container_size(pkg.CONTAINER_DDS, 18, h, w, n) == 0
    if n > 1:
        assert pkg.container_size(pkg.CONTAINER_PKM, 18, h, w, n) == 0


# ---- build check: the new kernels keep everything in registers

def test_etc2_rgb8_kernels_use_no_scratch(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    metas = {}
    for unit in ("etc2_rgb8_kernels.hip", "etc2_kernels.hip", "metric_kernels.hip"):
        out = os.path.join(str(tmp_path), unit + ".s")
        subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(T.ROOT, "include"),
                               "-I" + CSRC, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, unit)],
                              stderr=subprocess.DEVNULL)
        for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", open(out).read(), re.S):
            blk = m.group(0)
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            metas[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
    names = ["icamd_etc2_rgb8_%s%s_kernel" % (src, st) for src in ("rgb888", "rgba8") for st in ("", "_split_h", "_split_v", "_heuristic")]
    names += ["icamd_etc2_rgb8_decode_kernel", "icamd_metric_etc2_rgb8_rgb888_kernel", "icamd_metric_etc2_rgb8_rgba8_kernel",
              "icamd_etc2_rgba8_decode_kernel", "icamd_metric_etc2_rgba8_kernel"]  # (the last two now hold the complete decoder)
    for n in names:
        assert n in metas, n
        assert metas[n] == 0, "%s uses %d bytes of scratch" % (n, metas[n])
