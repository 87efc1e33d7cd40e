"""CPU tier for ICAMD_ETC2_RGB8A1, ETC2 RGB8 with punch-through alpha (include/ic_amd.h).

* The block math of image-compression_amd/csrc/etc2_a1_block.h compiled for the host (tests/host_emul/etc2_a1_emul.cc,
  -DICAMD_HOST_EMULATION), bit-exact against the numpy statement (tests/etc2_a1_oracle.py): the decoder in four modes under
  both opaque bits, the encoder under all four strategies.
* The hand words and the worked example of the header, as literals, through both.
* Exact properties of the encoder, and the classes of block the inputs must hold.
* The C ABI's host-side surface of codec 21: sizes, kernel names, container headers, the ICAMD_ERR_ARG cases.
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

import etc2_a1_oracle as A
import etc2_colour_oracle as C
import ic_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
pkg = importlib.import_module("image-compression_amd")
PADDED = [(30, 30, 40, 48), (5, 3, 16, 16), (1, 1, 9, 13), (64, 61, 64, 64), (17, 33, 24, 48)]  # as test_etc2_colour_host.py
MASKS = ("none", "blobs", "noise")
CASES = [(mask, h, w, gh, gw) for mask in MASKS for h, w, gh, gw in PADDED]

T_WORD = "1c0000f4ff00f0f0"  # T, Op = 0, C1 = (204, 0, 0), C2 = (0, 0, 255), d = 11
HALF_WORD = "6090c800ff000000"
# column x of every row, for the hand words of the header
KNOWN = {
    "00000000ffff0000": [(0, 0, 0, 0)] * 4,
    T_WORD: [(204, 0, 0, 255), (11, 11, 255, 255), (0, 0, 0, 0), (0, 0, 244, 255)],
    "1c0000f6ff00f0f0": [(204, 0, 0, 255), (11, 11, 255, 255), (0, 0, 255, 255), (0, 0, 244, 255)],
    HALF_WORD: [(99, 148, 206, 255), (99, 148, 206, 255), (0, 0, 0, 0), (0, 0, 0, 0)],
}


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("etc2a1") / "libetc2_a1_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC,
                           "-I" + os.path.join(T.ROOT, "include"), "-o", so, os.path.join(EMUL_DIR, "etc2_a1_emul.cc")])
    L = ctypes.CDLL(so)
    L.etc2a1_emul_encode.restype = ctypes.c_int
    L.etc2a1_emul_encode.argtypes = [T.ci, T.u32, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp]
    L.etc2a1_emul_decode_words.restype = None
    L.etc2a1_emul_decode_words.argtypes = [T.u32, T.ci, T.vp, T.vp]
    yield L
    T.assert_no_emul_violations(L, "test_etc2_a1_host")


def emul_decode_words(L, words, swap=0):
    b = np.frombuffer(bytes(words), np.uint8).copy()
    out = np.zeros((b.size // 8, 4, 4, 4), np.uint8)
    L.etc2a1_emul_decode_words(b.size // 8, swap, b.ctypes.data, out.ctypes.data)
    return out


def emul_encode(L, flat, h, w, strategy, gh=None, gw=None, stride=None):
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    out = np.zeros(A.encoded_size(gh, gw), np.uint8)
    src = np.ascontiguousarray(flat, dtype=np.uint8).reshape(-1)
    assert L.etc2a1_emul_encode(strategy, h, w, gh, gw, w * 4 if stride is None else stride, src.ctypes.data, out.ctypes.data)
    return out.tobytes()


@functools.lru_cache(maxsize=None)
def _image(mask, h, w):
    return A.masked_image("mixed", mask, h, w, index=h + w)


@functools.lru_cache(maxsize=None)
def _want(mask, h, w, gh, gw, strategy):
    return A.oracle_encode(_image(mask, h, w), h, w, 0, strategy, gh=gh, gw=gw, return_classes=True)


# ---- decoder

@pytest.mark.parametrize("word", sorted(KNOWN))
def test_hand_words(emul, word):
    b = bytes.fromhex(word)
    want = np.broadcast_to(np.array(KNOWN[word], np.uint8)[None, None], (1, 4, 4, 4))
    assert (A.decode_blocks(b) == want).all()
    assert (emul_decode_words(emul, b) == want).all()
    assert (emul_decode_words(emul, b, swap=1) == want[..., [2, 1, 0, 3]]).all()


def test_hand_word_modes():
    assert A.modes(bytes.fromhex(T_WORD)).tolist() == [A.T_MODE] and A.opaque_bit(bytes.fromhex(T_WORD)).tolist() == [0]
    assert A.modes(bytes.fromhex("1c0000f6ff00f0f0")).tolist() == [A.T_MODE]
    assert A.modes(bytes.fromhex(HALF_WORD)).tolist() == [A.DIFFERENTIAL]


def test_decoder_matches_statement_on_random_words(emul):
    n = 1 << 15
    words = A.random_words(4, 4 * n, seed=2100)
    seen = np.bincount(A.modes(words) * 2 + A.opaque_bit(words), minlength=2 * A.PLANAR + 2)
    assert (seen[2 * A.DIFFERENTIAL:] >= n // 16).all(), seen  # all four modes under both values of Op
    for swap in (0, 1):
        want = A.decode_blocks(words)
        assert (emul_decode_words(emul, words, swap) == (want[..., [2, 1, 0, 3]] if swap else want)).all()
    plain = np.frombuffer(T.random_blocks(T.ETC1, 4, 4 * n, seed=2101), np.uint8).reshape(-1, 8)  # no mode forced
    assert (emul_decode_words(emul, plain) == A.decode_blocks(plain)).all()


@pytest.mark.parametrize("mode", [A.T_MODE, A.H_MODE, A.PLANAR])
def test_decoder_on_constructed_words_with_op_0(emul, mode):
    n = 1 << 14
    words = np.frombuffer(A.random_words(4, 4 * n, seed=2110 + mode, only=mode, op=0), np.uint8).reshape(-1, 8)
    assert (A.modes(words) == mode).all() and not A.opaque_bit(words).any()
    got = emul_decode_words(emul, words)
    assert (got == A.decode_blocks(words)).all()
    rgb8 = words.copy()
    rgb8[:, 3] |= 2
    colour = C.decode_blocks(rgb8)
    if mode == A.PLANAR:  # alpha 255 everywhere, the colour of the ICAMD_ETC2_RGB8 word
        assert (got[..., 3] == 255).all() and (got[..., :3] == colour).all()
    else:  # exactly the texels of index 2 are holes
        hole = A._index_planes(C._words(words)[1]) == 2
        assert hole.any() and (got[hole] == 0).all() and (got[~hole][:, 3] == 255).all() and (got[~hole][:, :3] == colour[~hole]).all()


def test_op_1_differential_is_the_etc1_word(emul):
    n = 1 << 12
    words = np.frombuffer(A.random_words(4, 4 * n, seed=2120, only=A.DIFFERENTIAL, op=1), np.uint8).reshape(-1, 8)
    etc1 = T.oracle_decode(T.ETC1, words.tobytes(), 4, 4 * n).reshape(4, n, 4, 3).transpose(1, 0, 2, 3)
    got = emul_decode_words(emul, words)
    assert (got[..., :3] == etc1).all() and (got[..., 3] == 255).all()


# ---- encoder against the statement

def test_worked_example(emul):
    img = np.zeros((4, 4, 4), np.uint8)
    img[..., :3] = (100, 150, 200)
    img[:, :2, 3] = 255
    for strategy, word in ((0, "6090c801ff000000"), (1, HALF_WORD), (2, HALF_WORD), (3, HALF_WORD)):
        assert A.oracle_encode(img, 4, 4, 0, strategy).hex() == word
        assert emul_encode(emul, img, 4, 4, strategy).hex() == word
    _, err = A.search(img[None, ..., :3], img[None, ..., 3] >= 128, 0, 0)
    assert err.tolist() == [328] and A.search(img[None, ..., :3], img[None, ..., 3] >= 128, 0, 1)[1].tolist() == [328]
    img[..., 3] = 127
    for strategy in A.STRATEGIES:
        assert emul_encode(emul, img, 4, 4, strategy) == A.ALL_TRANSPARENT == A.oracle_encode(img, 4, 4, 0, strategy)


@pytest.mark.parametrize("mask,h,w,gh,gw", CASES)
def test_encoder_matches_statement(emul, mask, h, w, gh, gw):
    img = _image(mask, h, w)
    for strategy in A.STRATEGIES:
        want, info = _want(mask, h, w, gh, gw, strategy)
        got = emul_encode(emul, img, h, w, strategy, gh=gh, gw=gw)
        assert got == want, (mask, h, w, gh, gw, strategy)


def test_inputs_hold_every_class():
    classes, clamped, empty_sub, counts = set(), False, set(), set()
    for mask, h, w, gh, gw in CASES:
        for strategy in A.STRATEGIES:
            _, info = _want(mask, h, w, gh, gw, strategy)
            cls = info["class"]
            classes |= set(cls.tolist())
            through_d = (cls == A.D_OPAQUE) | (cls == A.D_MASKED)
            masked = cls == A.D_MASKED
            for flip in (0, 1):
                q5, cnt = A.search_bases(info["rgb"], info["opaque"], flip)
                d = q5[:, 1] - q5[:, 0]
                clamped = clamped or bool((through_d[:, None] & ((d < -4) | (d > 3))).any())
                if (masked & (cnt.min(axis=1) == 0)).any():
                    empty_sub.add(flip)
                counts |= set(cnt[masked].reshape(-1).tolist())
    # all-transparent, opaque with E differential, opaque with E individual (D with Op = 1), planar chosen, masked
    assert classes == {A.CLEAR, A.E_KEPT, A.D_OPAQUE, A.PLANAR_CHOSEN, A.D_MASKED}
    assert clamped                        # a delta outside the 3-bit range in at least one channel
    assert empty_sub == {0, 1}            # masked with one sub-block fully transparent, under each flip
    assert set(range(1, 8)) <= counts     # masked with n = 1..7 in a sub-block


@pytest.mark.parametrize("mask,h,w,gh,gw", CASES)
def test_encoder_properties(emul, mask, h, w, gh, gw):
    img = _image(mask, h, w)
    tex = A.block_texels(img, h, w, max(gh, h), max(gw, w))
    opq = tex[..., 3] >= 128
    full = opq.all(axis=(1, 2))
    for strategy in A.STRATEGIES:
        got = np.frombuffer(emul_encode(emul, img, h, w, strategy, gh=gh, gw=gw), np.uint8).reshape(-1, 8)
        dec = A.decode_blocks(got)
        assert (dec[..., 3] == np.where(opq, 255, 0)).all()                      # alpha is the mask, texel by texel
        assert ((A.opaque_bit(got) == 1) | (A.modes(got) == A.PLANAR))[full].all()  # an opaque block never carries Op = 0
        assert (A.modes(got)[~full] == A.DIFFERENTIAL).all()                     # no planar candidate beside transparency
        if full.any():
            e = np.frombuffer(T.oracle_encode(T.ETC1, img, h, w, 4, 0, strategy, gh=max(gh, h), gw=max(gw, w)), np.uint8).reshape(-1, 8)
            rgb8 = np.frombuffer(C.oracle_encode(img, h, w, 4, 0, strategy, gh=gh, gw=gw), np.uint8).reshape(-1, 8)
            same = full & ((e[:, 3] & 2) != 0)
            assert (got[same] == rgb8[same]).all()                               # E differential: the ICAMD_ETC2_RGB8 bytes
            _, info = _want(mask, h, w, gh, gw, strategy)
            sse_c = C.sse(tex[full][..., :3], C.decode_blocks(info["c_words"][full]))
            assert (C.sse(tex[full][..., :3], dec[full][..., :3]) <= sse_c).all()  # never worse than C


def test_row_padding_and_swap_do_not_enter(emul):
    h, w, pad = 13, 22, 5
    img = A.masked_image("smooth", "blobs", h, w, index=3)
    flat = T.with_row_padding(img, pad)
    for swap in (0, 1):  # (swap_rb never reaches the block math: bytes 0..2 as they lie in memory)
        assert emul_encode(emul, flat, h, w, 2, stride=w * 4 + pad) == A.oracle_encode(img, h, w, swap, 2)


# ---- the C ABI's host-side surface (no device work: every check below returns before the GPU is touched)

def test_codec_value_sizes_and_kernel_names():
    assert pkg.ETC2_RGB8A1 == 21 == A.ETC2_RGB8A1
    assert pkg.encoded_size(21, 8, 8) == 32 and pkg.encoded_size(21, 5, 3) == 16
    assert pkg.encoded_size(21, 257, 1023) == 65 * 256 * 8
    assert pkg.kernel_name(21, 4) == "icamd_etc2_rgb8a1_kernel"
    assert pkg.kernel_name(21, 3) == "" and pkg.kernel_name(21, 5) == ""
    assert pkg.metric_kernel_name(21, 4) == "icamd_metric_etc2_rgb8a1_kernel"
    assert pkg.metric_kernel_name(21, 3) == ""
    assert pkg.mip_chain_size(21, 64, 64, 3) == (0, None) and pkg.mip_kernel_name(21, 4) == ""
    assert pkg.kernel_name(pkg.ETC2_RGBA8, 4) == "icamd_etc2_rgba8_kernel"  # unchanged
    assert pkg.kernel_name(pkg.ETC2_RGB8, 4) == "icamd_etc2_rgb8_rgba8_kernel"


def test_argument_errors():
    lib = pkg.lib()
    dummy = ctypes.c_void_p(16)  # never dereferenced: the arguments are refused first
    for comps in (0, 1, 2, 3, 5):
        assert lib.icamd_encode_device(21, 2, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, dummy, dummy, None) == -4, comps
        assert lib.icamd_measure_error_device(21, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, dummy, dummy, dummy, None) == -4, comps
    assert lib.icamd_encode_device(21, 2, 4, 0, 0, 8, 8, 8, 32, 1, 0, 0, dummy, dummy, None) == 1    # empty image
    assert lib.icamd_encode_device(21, 2, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, None, dummy, None) == 1     # null source
    assert lib.icamd_decode_device(21, 0, 8, 0, 0, 1, 0, 0, dummy, dummy, None) == 1
    assert lib.icamd_decode_device(21, 0, 8, 8, 0, 1, 0, 0, None, dummy, None) == 1
    assert lib.icamd_measure_error_device(21, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, dummy, None, dummy, None) == 1
    assert lib.icamd_measure_error_device(21, 4, 0, 8, 8, 8, 8, 31, 1, 0, 0, dummy, dummy, dummy, None) == -4  # stride < row
    assert lib.icamd_measure_error_device(21, 4, 0, 8, 8, 4, 8, 32, 1, 0, 0, dummy, dummy, dummy, None) == -4  # grid < image
    # the mip entry points, as for the other ETC2 codecs
    assert lib.icamd_encode_mips_device(21, 2, 4, 0, 8, 8, 32, 1, 1, 0, 0, dummy, dummy, None, 0, None) == -4
    assert lib.icamd_encode_mips_filtered_device(21, 2, 4, 0, 0, 8, 8, 32, 1, 1, 0, 0, dummy, dummy, None, 0, None) == -4
    assert pkg.lib().icamd_mip_workspace_size(21, 4, 64, 64, 3, 1) == 0


def test_17_and_22_are_unassigned():
    lib = pkg.lib()
    dummy = ctypes.c_void_p(16)
    for codec in (17, 22):
        assert pkg.kernel_name(codec, 3) == "" and pkg.kernel_name(codec, 4) == "" and pkg.metric_kernel_name(codec, 4) == ""
        assert lib.icamd_decode_device(codec, 0, 8, 8, 0, 1, 0, 0, dummy, dummy, None) == 1
        assert lib.icamd_measure_error_device(codec, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, dummy, dummy, dummy, None) == -4
        for container in (pkg.CONTAINER_DDS, pkg.CONTAINER_KTX, pkg.CONTAINER_PKM, pkg.CONTAINER_PVR):
            assert pkg.container_size(container, codec, 8, 8, 1) == 0


def test_host_buffer_entry_points_do_not_reach_the_codec():
    lib = pkg.lib()
    for fmt in (pkg.RGB, pkg.BGR, pkg.RGBA, pkg.BGRA):
        assert lib.icamd_supports_format(pkg.COMPRESSOR_ETC, fmt) == (1 if fmt == pkg.RGB else 0)
    assert pkg.compute_compressed_data_size(pkg.COMPRESSOR_ETC, pkg.RGBA, 8, 8) == 0


def _levels(h, w, n):
    g = np.random.default_rng(210 + n)
    return [g.integers(0, 256, ((max(1, h >> l) + 3) // 4) * ((max(1, w >> l) + 3) // 4) * 8, dtype=np.uint8).tobytes()
            for l in range(n)]


def _ktx(h, w, levels):
    return bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A]) + \
        struct.pack("<13I", 0x04030201, 0, 1, 0, 0x9276, 0x1908, w, h, 0, 0, 1, len(levels), 0) + \
        b"".join(struct.pack("<I", len(b)) + b for b in levels)


def _pvr(h, w, levels):
    return struct.pack("<IIQIIIIIIIII", 0x03525650, 0, 24, 0, 0, h, w, 1, 1, 1, len(levels), 0) + b"".join(levels)


def _pkm(h, w, levels):
    return b"PKM 20" + struct.pack(">HHHHH", 4, (w + 3) & ~3, (h + 3) & ~3, w, h) + levels[0]


@pytest.mark.parametrize("h,w,n", [(64, 64, 1), (64, 64, 7), (61, 59, 3), (5, 3, 1)])
def test_container_bytes(h, w, n):
    levels = _levels(h, w, n)
    cases = [(pkg.CONTAINER_KTX, _ktx(h, w, levels)), (pkg.CONTAINER_PVR, _pvr(h, w, levels))]
    if n == 1:
        cases.append((pkg.CONTAINER_PKM, _pkm(h, w, levels)))
    for container, want in cases:
        assert pkg.container_size(container, 21, h, w, n) == len(want)
        assert pkg.container_write(container, 21, h, w, levels) == want, (container, h, w, n)
    assert pkg.container_size(pkg.CONTAINER_DDS, 21, h, w, n) == 0
    if n > 1:
        assert pkg.container_size(pkg.CONTAINER_PKM, 21, h, w, n) == 0


# ---- build check: the new kernels keep everything in registers

def test_etc2_a1_kernels_use_no_scratch(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    metas = {}
    for unit in ("etc2_a1_kernels.hip", "metric_kernels.hip"):
        out = os.path.join(str(tmp_path), unit + ".s")
        subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(T.ROOT, "include"),
                               "-I" + CSRC, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, unit)],
                              stderr=subprocess.DEVNULL)
        for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", open(out).read(), re.S):
            blk = m.group(0)
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            metas[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
    names = ["icamd_etc2_rgb8a1%s_kernel" % st for st in ("", "_split_h", "_split_v", "_heuristic")]
    names += ["icamd_etc2_rgb8a1_decode_kernel", "icamd_metric_etc2_rgb8a1_kernel"]
    for n in names:
        assert n in metas, n
        assert metas[n] == 0, "%s uses %d bytes of scratch" % (n, metas[n])
