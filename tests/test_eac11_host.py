"""CPU tier for the EAC R11 / RG11 extension (include/ic_amd.h, ICAMD_EAC_R11).

* The block math of image-compression_amd/csrc/eac11_block.h compiled for the host (tests/host_emul/eac11_emul.cc,
  -DICAMD_HOST_EMULATION), bit-exact against the numpy definition (tests/eac11_oracle.py) for every source layout.
* The pin: R11 of an image's alpha plane is bytes 0..7 of the ETC2 RGBA8 definition's blocks.
* The 11-bit decoder: the header's hand words, random words, where it equals the alpha decoder and where it does not.
* The C ABI's host-side surface: sizes, kernel names, the ICAMD_ERR_ARG / ICAMD_FALSE cases, mip refusal, container framing.
* The new kernels compile without scratch."""
import ctypes
import functools
import importlib
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bc45_oracle as B
import eac11_oracle as A
import etc2_oracle as E
import ic_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
pkg = importlib.import_module("image-compression_amd")
PADDED = [(30, 30, 40, 48), (5, 3, 16, 16), (1, 1, 9, 13), (64, 61, 64, 64), (17, 33, 24, 48)]
R11, RG11 = A.EAC_R11, A.EAC_RG11
LARGEST = max(range(len(B.SHAPES)), key=lambda i: B.SHAPES[i][0] * B.SHAPES[i][1])


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("eac11") / "libeac11_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC,
                           "-I" + os.path.join(T.ROOT, "include"), "-o", so, os.path.join(EMUL_DIR, "eac11_emul.cc")])
    L = ctypes.CDLL(so)
    L.eac11_emul_encode.restype = ctypes.c_int
    L.eac11_emul_encode.argtypes = [T.ci, T.ci, T.ci, T.u32, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp]
    L.eac11_emul_decode.restype = ctypes.c_int
    L.eac11_emul_decode.argtypes = [T.ci, T.u32, T.u32, T.u32, T.vp, T.vp]
    yield L
    T.assert_no_emul_violations(L, "test_eac11_host")


def emul_encode(L, codec, flat, h, w, comps, swap=0, gh=None, gw=None, stride=None):
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    out = np.zeros(A.encoded_size(codec, gh, gw), np.uint8)
    src = np.ascontiguousarray(flat, dtype=np.uint8).reshape(-1)
    assert L.eac11_emul_encode(int(codec == RG11), comps, swap, h, w, gh, gw, w * comps if stride is None else stride,
                               src.ctypes.data, out.ctypes.data)
    return out.tobytes()


def emul_decode(L, codec, blocks, h, w, pad=0):
    out = np.zeros(h * (w * A.comps_out(codec) + pad), np.uint8)
    b = np.frombuffer(bytes(blocks), np.uint8).copy()
    assert L.eac11_emul_decode(int(codec == RG11), h, w, pad, b.ctypes.data, out.ctypes.data)
    return out


def emul_decode_words(L, words):
    """[n, 8] words -> [n, 16] decoded bytes, texel i = 4 x + y (the words as the blocks of a 4 x 4 n R11 image)."""
    n = words.shape[0]
    plane = emul_decode(L, R11, words.tobytes(), 4, 4 * n).reshape(4, n, 4)  # [y, block, x]
    return plane.transpose(1, 2, 0).reshape(n, 16).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _channel_words(gen, shape_index, ch):
    """The definition's words of channel ch of the (gen, shape) test image: computed once, shared by every layout."""
    h, w, _ = B.SHAPES[shape_index]
    return A.channel_words(B.image(gen, h, w, 4, index=shape_index)[..., ch], h, w)


def _want(codec, gen, shape_index, comps, swap):
    r = _channel_words(gen, shape_index, 2 if (swap and comps >= 3) else 0)
    if codec == R11:
        return r.tobytes()
    return np.concatenate([r, _channel_words(gen, shape_index, 1)], axis=1).tobytes()


# ---- encoder against the definition

@pytest.mark.parametrize("gen", sorted(B.GENERATORS))
def test_encoder_matches_definition_on_every_shape_and_layout(emul, gen):
    for i, (h, w, pad) in enumerate(B.SHAPES):
        if i == LARGEST and gen != "mixed":  # (the numpy search takes seconds there: once)
            continue
        for codec, comps, swap in A.LAYOUTS:
            img = B.image(gen, h, w, comps, index=i)
            flat = T.with_row_padding(img, pad)
            got = emul_encode(emul, codec, flat, h, w, comps, swap, stride=w * comps + pad)
            assert got == _want(codec, gen, i, comps, swap), (gen, h, w, pad, codec, comps, swap)
            if i < 2 and gen == "mixed":  # the shared words are what oracle_encode states
                assert got == A.oracle_encode(codec, img, h, w, comps, swap)


@pytest.mark.parametrize("h,w,gh,gw", PADDED)
def test_encoder_padded_grid(emul, h, w, gh, gw):
    for gen in ("noise", "saturated"):
        for codec, comps, swap in A.LAYOUTS:
            img = B.image(gen, h, w, comps, index=h + w)
            want = A.oracle_encode(codec, img, h, w, comps, swap, gh=gh, gw=gw)
            assert emul_encode(emul, codec, img, h, w, comps, swap, gh=gh, gw=gw) == want, (gen, h, w, gh, gw, codec, comps, swap)


@pytest.mark.parametrize("h,w,gh,gw", [(61, 59, 61, 59), (64, 64, 64, 64), (5, 3, 5, 3)] + PADDED)
def test_r11_is_the_alpha_half_of_etc2_rgba8(emul, h, w, gh, gw):
    img = B.image("mixed", h, w, 4, index=h * w)
    etc2 = np.frombuffer(E.oracle_encode(img, h, w, 0, T.HEURISTIC, gh=gh, gw=gw), np.uint8).reshape(-1, 16)
    alpha = np.ascontiguousarray(img[..., 3])
    assert emul_encode(emul, R11, alpha, h, w, 1, gh=gh, gw=gw) == etc2[:, :8].tobytes()


def test_encoder_every_range(emul):
    strip = E.every_range_strip()
    h, w = strip.shape
    got = emul_encode(emul, R11, strip, h, w, 1)
    assert got == A.oracle_encode(R11, strip, h, w, 1)
    mult = np.frombuffer(got, np.uint8).reshape(-1, 8)[:, 1] >> 4
    assert (mult != 0).all()


def test_encoder_never_writes_multiplier_zero(emul):
    for gen in sorted(B.GENERATORS):
        h, w, _ = B.SHAPES[1]
        img = B.image(gen, h, w, 2, index=3)
        words = np.frombuffer(emul_encode(emul, RG11, img, h, w, 2), np.uint8).reshape(-1, 8)
        assert ((words[:, 1] >> 4) != 0).all(), gen


def test_flat_and_0_255_blocks_decode_exactly(emul):
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9500))
    flat = np.repeat(np.arange(256, dtype=np.uint8), 4)[None, :].repeat(4, axis=0)  # 4 x 1024: block i is all i
    binary = (g.integers(0, 2, size=(4, 1024)) * 255).astype(np.uint8)
    binary[:, :4], binary[:, 4:8] = 0, 255
    for plane in (flat, binary):
        h, w = plane.shape
        words = emul_encode(emul, R11, plane, h, w, 1)
        assert ((np.frombuffer(words, np.uint8).reshape(-1, 8)[:, 1] >> 4) != 0).all()
        assert (emul_decode(emul, R11, words, h, w).reshape(h, w) == plane).all()


# ---- decoder

HAND_WORDS = [
    ("80 0d 7e 49 24 92 49 24", [127, 129] + [128] * 14, [1018, 1037] + [1028] * 14),  # base 128, multiplier 0, table 13
    ("ff 00 ff ff ff ff ff ff", [255] * 16, [2047] * 16),                               # base 255, table 0, index 7: clamps
    ("00 00 6d b6 db 6d b6 db", [0] * 16, [0] * 16),                                    # base 0, table 0, index 3: clamps
]


def test_decoder_hand_words(emul):
    words = np.array([[int(b, 16) for b in text.split()] for text, _, _ in HAND_WORDS], np.uint8)
    assert A.eac11_decode_v11(words).tolist() == [v11 for _, _, v11 in HAND_WORDS]
    assert A.eac11_decode(words).tolist() == [byte for _, byte, _ in HAND_WORDS]
    assert emul_decode_words(emul, words).tolist() == [byte for _, byte, _ in HAND_WORDS]
    assert (E.eac_decode(words[:1]) == 128).all()  # the alpha decoder on the first word: base everywhere


def test_decoder_matches_definition(emul):
    for i, (h, w, pad) in enumerate(B.SHAPES[:-1]):
        for codec in (R11, RG11):
            words = A.random_words(codec, h, w, seed=500 + i)
            al = np.frombuffer(words, np.uint8).reshape(-1, 8)
            if al.shape[0] >= 8:
                assert ((al[:, 1] >> 4) == 0).any() and (al[:, 0] == 0).any() and (al[:, 0] == 255).any()
            assert emul_decode(emul, codec, words, h, w, pad).tobytes() == A.oracle_decode(codec, words, h, w, pad).tobytes(), (h, w, codec)


def test_decoder_against_the_alpha_decoder(emul):
    words = np.frombuffer(A.random_words(R11, 256, 256, seed=77), np.uint8).reshape(-1, 8)
    mult = words[:, 1] >> 4
    got, alpha = emul_decode_words(emul, words), E.eac_decode(words)
    assert (got == A.eac11_decode(words)).all()
    assert (got[mult != 0] == alpha[mult != 0]).all()  # multiplier >= 1: the alpha decoder's bytes
    zero = mult == 0
    assert zero.sum() >= 1000
    diff = np.abs(got[zero] - alpha[zero])
    assert diff.max() <= 2  # (4 + M) >> 3 with M in -15 .. 14
    assert (diff.max(axis=1) > 0).mean() > 0.99


# ---- the C ABI's host-side surface (no device work: every check below returns before the GPU is touched)

NAMES = {(R11, 1): "icamd_eac_r11_r8_kernel", (R11, 2): "icamd_eac_r11_rg8_kernel", (R11, 3): "icamd_eac_r11_rgb888_kernel",
         (R11, 4): "icamd_eac_r11_rgba8_kernel", (RG11, 2): "icamd_eac_rg11_rg8_kernel", (RG11, 3): "icamd_eac_rg11_rgb888_kernel",
         (RG11, 4): "icamd_eac_rg11_rgba8_kernel"}


def test_codec_values_sizes_and_kernel_names():
    assert (pkg.EAC_R11, pkg.EAC_RG11) == (19, 20) == (R11, RG11)
    assert pkg.encoded_size(R11, 8, 8) == 32 and pkg.encoded_size(RG11, 8, 8) == 64
    assert pkg.encoded_size(R11, 5, 3) == 16 and pkg.encoded_size(RG11, 5, 3) == 32
    assert pkg.encoded_size(R11, 257, 1023) == 65 * 256 * 8 and pkg.encoded_size(RG11, 257, 1023) == 65 * 256 * 16
    for codec in (R11, RG11):
        for comps in range(0, 6):
            name = NAMES.get((codec, comps), "")
            assert pkg.kernel_name(codec, comps) == name, (codec, comps)
            assert pkg.metric_kernel_name(codec, comps) == name.replace("icamd_", "icamd_metric_"), (codec, comps)
        assert pkg.mip_chain_size(codec, 64, 64, 3) == (0, None)
        assert pkg.mip_kernel_name(codec, 4) == ""
        assert pkg.lib().icamd_mip_workspace_size(codec, 4, 64, 64, 3, 1) == 0


def test_argument_errors():
    lib = pkg.lib()
    dummy = ctypes.c_void_p(16)  # never dereferenced: the arguments are refused first
    for codec in (R11, RG11):
        for comps in range(0, 6):
            ok = (codec, comps) in NAMES
            stride = 8 * max(comps, 1)
            for swap in (0, 1):
                # (no images: an accepted call answers ICAMD_OK after its checks and launches nothing)
                want = -4 if (not ok or (swap and comps < 3)) else 0
                for n in ((0, 1) if want else (0,)):
                    st = lib.icamd_encode_device(codec, 2, comps, swap, 8, 8, 8, 8, stride, n, 0, 0, dummy, dummy, None)
                    assert st == want, (codec, comps, swap, n, st)
                    st = lib.icamd_measure_error_device(codec, comps, swap, 8, 8, 8, 8, stride, n, 0, 0, dummy, dummy, dummy, None)
                    assert st == want, (codec, comps, swap, n, st)
        comps = 2
        assert lib.icamd_encode_device(codec, 2, comps, 0, 8, 8, 8, 8, 15, 1, 0, 0, dummy, dummy, None) == -4  # stride < row
        assert lib.icamd_encode_device(codec, 2, comps, 0, 0, 8, 8, 8, 16, 1, 0, 0, dummy, dummy, None) == 1   # empty image
        assert lib.icamd_encode_device(codec, 2, comps, 0, 8, 8, 8, 8, 16, 1, 0, 0, None, dummy, None) == 1    # null source
        assert lib.icamd_encode_device(codec, 2, comps, 0, 8, 8, 8, 8, 16, 0, 0, 0, dummy, dummy, None) == 0   # no images
        assert lib.icamd_decode_device(codec, 1, 8, 8, 0, 1, 0, 0, dummy, dummy, None) == -4                   # swap_rb
        assert lib.icamd_decode_device(codec, 0, 8, 0, 0, 1, 0, 0, dummy, dummy, None) == 1
        assert lib.icamd_decode_device(codec, 0, 8, 8, 0, 0, 0, 0, dummy, dummy, None) == 0
        assert lib.icamd_measure_error_device(codec, comps, 0, 8, 8, 8, 8, 15, 1, 0, 0, dummy, dummy, dummy, None) == -4  # stride
        assert lib.icamd_measure_error_device(codec, comps, 0, 8, 8, 4, 8, 16, 1, 0, 0, dummy, dummy, dummy, None) == -4  # grid
        assert lib.icamd_measure_error_device(codec, comps, 0, 8, 8, 8, 8, 16, 1, 0, 0, dummy, dummy, ctypes.c_void_p(20), None) == -4
        # the mip entry points refuse the codecs, as they do ETC2
        assert lib.icamd_encode_mips_device(codec, 2, 4, 0, 8, 8, 32, 1, 1, 0, 0, dummy, dummy, None, 0, None) == -4
        assert lib.icamd_encode_mips_filtered_device(codec, 2, 4, 0, 0, 8, 8, 32, 1, 1, 0, 0, dummy, dummy, None, 0, None) == -4


def test_compressor_format_mapping_is_unchanged():
    lib = pkg.lib()
    for comp in (pkg.COMPRESSOR_DXTC, pkg.COMPRESSOR_ETC, pkg.COMPRESSOR_PVRTC):
        for fmt in (pkg.RGB, pkg.BGR, pkg.RGBA, pkg.BGRA):
            want = 1 if comp == pkg.COMPRESSOR_DXTC else int(fmt == (pkg.RGB if comp == pkg.COMPRESSOR_ETC else pkg.RGBA))
            assert lib.icamd_supports_format(comp, fmt) == want


def _levels(codec, h, w, n):
    g = np.random.default_rng(190 + n)
    return [g.integers(0, 256, A.encoded_size(codec, max(1, h >> l), max(1, w >> l)), dtype=np.uint8).tobytes() for l in range(n)]


def _ktx(codec, h, w, levels):
    internal, base = (0x9270, 0x1903) if codec == R11 else (0x9272, 0x8227)
    return bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A]) + \
        struct.pack("<13I", 0x04030201, 0, 1, 0, internal, base, w, h, 0, 0, 1, len(levels), 0) + \
        b"".join(struct.pack("<I", len(b)) + b for b in levels)


def _pvr(codec, h, w, levels):
    return struct.pack("<IIQIIIIIIIII", 0x03525650, 0, 25 if codec == R11 else 26, 0, 0, h, w, 1, 1, 1, len(levels), 0) + b"".join(levels)


def _pkm(codec, h, w, levels):
    return b"PKM 20" + struct.pack(">HHHHH", 5 if codec == R11 else 6, (w + 3) & ~3, (h + 3) & ~3, w, h) + levels[0]


@pytest.mark.parametrize("codec", [R11, RG11])
@pytest.mark.parametrize("h,w,n", [(64, 64, 1), (64, 64, 7), (61, 59, 3), (5, 3, 1), (256, 128, 9)])
def test_container_bytes(codec, h, w, n):
    levels = _levels(codec, h, w, n)
    cases = [(pkg.CONTAINER_KTX, _ktx(codec, h, w, levels)), (pkg.CONTAINER_PVR, _pvr(codec, h, w, levels))]
    if n == 1:
        cases.append((pkg.CONTAINER_PKM, _pkm(codec, h, w, levels)))
    for container, want in cases:
        assert pkg.container_size(container, codec, h, w, n) == len(want)
        assert pkg.container_write(container, codec, h, w, levels) == want, (container, h, w, n)
    assert pkg.container_size(pkg.CONTAINER_DDS, codec, h, w, n) == 0
    if n > 1:
        assert pkg.container_size(pkg.CONTAINER_PKM, codec, h, w, n) == 0


# ---- build check: the new kernels keep everything in registers

def test_eac11_kernels_use_no_scratch(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    metas = {}
    for unit in ("eac11_kernels.hip", "metric_kernels.hip"):
        out = os.path.join(str(tmp_path), unit + ".s")
        subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(T.ROOT, "include"),
                               "-I" + CSRC, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, unit)],
                              stderr=subprocess.DEVNULL)
        for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", open(out).read(), re.S):
            blk = m.group(0)
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            metas[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
    names = sorted(NAMES.values()) + [n.replace("icamd_", "icamd_metric_") for n in NAMES.values()] + \
        ["icamd_eac_r11_decode_kernel", "icamd_eac_rg11_decode_kernel"]
    for n in names:
        assert n in metas, n
        assert metas[n] == 0, "%s uses %d bytes of scratch" % (n, metas[n])
