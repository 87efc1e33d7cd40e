"""CPU tier: the per-block kernel math (image-compression_amd/csrc/*_block.h) compiled for the host with
the gfx950 instruction wrappers emulated (tests/host_emul), checked against the oracle.  This is NOT a
product path -- it only lets kernel-logic regressions show up without a GPU; the real parity tests are
tests/test_gpu_parity.py (-m gpu) which run the HIP kernels through the C ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ic_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")


@pytest.fixture(scope="module")
def emul():
    so = os.path.join(EMUL_DIR, "libic_emul.so")
    srcs = [os.path.join(EMUL_DIR, "emul.cc")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION",
                               "-I" + CSRC, "-o", so, os.path.join(EMUL_DIR, "emul.cc")])
    L = ctypes.CDLL(so)
    L.emul_encode.restype = ctypes.c_int
    L.emul_encode.argtypes = [T.ci, T.ci, T.ci, T.ci, T.u32, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp]
    yield L
    T.assert_no_emul_violations(L, "test_kernel_math_host")


def emul_encode(L, codec, src, h, w, comps, swap=0, strategy=2, gh=None, gw=None, stride=None):
    gh = h if gh is None else gh
    gw = w if gw is None else gw
    stride = w * comps if stride is None else stride
    n = T.oracle().ico_encoded_size(codec, max(gh, h), max(gw, w))
    out = np.zeros(n, np.uint8)
    src = np.ascontiguousarray(src, dtype=np.uint8)
    # over-allocate: interior loads read 16 B per row even for the last pixel
    buf = np.concatenate([src.reshape(-1), np.zeros(64, np.uint8)])
    ok = L.emul_encode(codec, strategy, comps, swap, h, w, gh, gw, stride, buf.ctypes.data, out.ctypes.data)
    return out.tobytes() if ok else None


CASES = [(T.DXT1, 3, 0, 2), (T.DXT1, 3, 1, 2), (T.DXT1, 4, 0, 2), (T.DXT1, 4, 1, 2), (T.DXT5, 4, 0, 2),
         (T.DXT5, 4, 1, 2), (T.ETC1, 3, 0, 0), (T.ETC1, 3, 0, 1), (T.ETC1, 3, 0, 2), (T.ETC1, 3, 0, 3),
         (T.ETC1, 4, 0, 2), (T.ETC1, 4, 0, 3)]


@pytest.mark.parametrize("codec,comps,swap,strategy", CASES)
@pytest.mark.parametrize("gen", ["noise", "smooth", "flat", "mixed"])
def test_block_math_matches_oracle(emul, codec, comps, swap, strategy, gen):
    for (h, w, pad) in [(64, 64, 0), (61, 59, 3), (5, 3, 0), (1, 1, 0)]:
        img = T.GENERATORS[gen](h, w, comps, index=h * 7 + w)
        src = T.with_row_padding(img, pad)
        stride = w * comps + pad
        want = T.oracle_encode(codec, src, h, w, comps, swap, strategy, stride=stride)
        got = emul_encode(emul, codec, src, h, w, comps, swap, strategy, stride=stride)
        assert got == want, (gen, h, w, pad)


@pytest.mark.parametrize("codec,comps,swap,strategy", CASES)
def test_block_math_pad_grid(emul, codec, comps, swap, strategy):
    img = T.s_mixed(30, 30, comps, index=60)
    src = T.with_row_padding(img, 8)
    want = T.oracle_encode(codec, src, 30, 30, comps, swap, strategy, gh=40, gw=48, stride=30 * comps + 8)
    got = emul_encode(emul, codec, src, 30, 30, comps, swap, strategy, gh=40, gw=48, stride=30 * comps + 8)
    assert got == want


def test_block_math_random_blocks(emul):
    g = np.random.Generator(np.random.PCG64(7))
    n = 1 << 14
    for codec, comps, swap, strategy in CASES:
        strip = g.integers(0, 256, size=(4, 4 * n, comps), dtype=np.uint8)
        base = g.integers(0, 256, size=(1, n // 2, 1, comps), dtype=np.int64)
        jit = g.integers(-3, 4, size=(4, n // 2, 4, comps), dtype=np.int64)
        strip[:, : 2 * n] = np.clip(base + jit, 0, 255).astype(np.uint8).reshape(4, 2 * n, comps)
        # extremes: make some blocks saturate the ETC clamps
        strip[:, 2 * n: 2 * n + 256] = g.choice(np.array([0, 1, 254, 255], np.uint8), size=(4, 256, comps))
        want = T.oracle_encode(codec, strip, 4, 4 * n, comps, swap, strategy)
        got = emul_encode(emul, codec, strip, 4, 4 * n, comps, swap, strategy)
        assert got == want, (codec, comps, swap, strategy)


def dxt_boundary_blocks(g, n, comps):
    """n 4x4 blocks (as a 4 x 4n strip) built to sit ON the decision boundaries of the DXT colour index search: every
    pixel is an endpoint, a /3 blend or a midpoint between neighbouring palette entries of two random endpoint colours,
    plus a jitter of 0 .. +-2; the endpoint distance ranges from 0 (constant path, degenerate palettes whose blends
    reorder under truncation) to the full cube."""
    e0 = g.integers(0, 256, size=(n, 1, 3), dtype=np.int64)
    spread = g.choice(np.array([0, 1, 2, 3, 4, 6, 9, 14, 27, 40, 80, 255]), size=(n, 1, 1))
    e1 = np.clip(e0 + g.integers(-1, 2, size=(n, 1, 3)) * spread + g.integers(-2, 3, size=(n, 1, 3)), 0, 255)
    num = g.choice(np.array([0, 1, 2, 3, 4, 5, 6]), size=(n, 16, 1))  # position on the segment in sixths
    px = (e0 * (6 - num) + e1 * num) // 6 + g.integers(-2, 3, size=(n, 16, 1)) * (g.integers(0, 3, size=(n, 1, 1)) == 0)
    px = np.clip(px, 0, 255).astype(np.uint8)
    # make sure both endpoints occur
    px[:, 0, :] = e0[:, 0, :]
    px[:, 15, :] = e1[:, 0, :]
    if comps == 4:
        px = np.concatenate([px, g.integers(0, 256, size=(n, 16, 1), dtype=np.uint8)], axis=2)
    # block b, pixel (y, x) -> strip[y, 4 b + x]
    return np.ascontiguousarray(px.reshape(n, 4, 4, comps).transpose(1, 0, 2, 3).reshape(4, 4 * n, comps))


def test_dxt_color_index_search_on_decision_boundaries(emul):
    """The O(1) colour index search of dxt_block.h (sorted-palette thresholds, r03) and its fall-back scan against the
    oracle's four-candidate scan (dxtc.cc:315-349) on blocks constructed to hit ties and degenerate palettes."""
    g = np.random.Generator(np.random.PCG64(303))
    n = 1 << 17
    for codec, comps, swap in ((T.DXT1, 3, 0), (T.DXT1, 3, 1), (T.DXT1, 4, 0), (T.DXT5, 4, 0), (T.DXT5, 4, 1)):
        strip = dxt_boundary_blocks(g, n, comps)
        want = T.oracle_encode(codec, strip, 4, 4 * n, comps, swap, 2)
        got = emul_encode(emul, codec, strip, 4, 4 * n, comps, swap, 2)
        if got != want:
            bb = 16 if codec == T.DXT5 else 8
            bad = [i for i in range(n) if got[i * bb:(i + 1) * bb] != want[i * bb:(i + 1) * bb]]
            raise AssertionError((codec, comps, swap, len(bad), bad[:5]))


def test_pvrtc_math_matches_oracle(emul):
    for n in (8, 16, 32, 64, 128):
        for gen in ("noise", "smooth", "flat", "mixed"):
            img = T.GENERATORS[gen](n, n, 4, index=n)
            want = T.oracle_encode(T.PVRTC2, img, n, n, 4)
            got = emul_encode(emul, T.PVRTC2, img, n, n, 4)
            assert got == want, (n, gen)
    img = np.zeros((32, 32, 4), np.uint8)  # never-updated maxima refer to image pixel 0
    img[0, 0] = (250, 3, 7, 255)
    img[8:, :, 1] = 200
    img[:, 16:, 3] = 255
    assert emul_encode(emul, T.PVRTC2, img, 32, 32, 4) == T.oracle_encode(T.PVRTC2, img, 32, 32, 4)


def test_pvrtc4_math_matches_oracle(emul):
    """PVRTC 4 bpp (extension, parity unpinned): the device block math (pvrtc4_extremes, pvrtc4_block_data) against the
    oracle's restatement of the same rules -- two independent forms of one specification, not a reference check."""
    for n in (8, 16, 32, 64, 128):
        for gen in ("noise", "smooth", "flat", "mixed"):
            img = T.GENERATORS[gen](n, n, 4, index=n + 4)
            assert emul_encode(emul, T.PVRTC4, img, n, n, 4) == T.oracle_encode(T.PVRTC4, img, n, n, 4), (n, gen)
    img = np.zeros((32, 32, 4), np.uint8)  # never-updated maxima refer to image pixel 0
    img[0, 0] = (250, 3, 7, 255)
    img[8:, :, 1] = 200
    img[:, 16:, 3] = 255
    assert emul_encode(emul, T.PVRTC4, img, 32, 32, 4) == T.oracle_encode(T.PVRTC4, img, 32, 32, 4)


def test_pvrtc4_round_trip_properties():
    """What ties the (reference-less) 4 bpp pair to the format: a solid texture decodes to the encoder's channel-reduced
    colour; a clean gradient survives at high PSNR; 4 bpp is at least as close to the source as 2 bpp on every content."""
    def psnr(a, b):
        mse = float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())
        return 99.0 if mse == 0 else 10 * np.log10(255.0 * 255.0 / mse)
    n = 64
    # colour A keeps R5 G5 B4, colour B R5 G5 B5 of an opaque colour (pvrtc.cc:337-349): a solid texture decodes to ONE colour
    # that lies between the two reduced colours and is never further from the source than colour A
    for colour, red_a, red_b in (((200, 100, 50, 255), (206, 99, 51, 255), (206, 99, 49, 255)),
                                 ((16, 255, 0, 255), (16, 255, 0, 255), (16, 255, 0, 255))):
        img = np.empty((n, n, 4), np.uint8)
        img[:] = colour
        dec = T.oracle_decode(T.PVRTC4, T.oracle_encode(T.PVRTC4, img, n, n, 4), n, n).reshape(-1, 4)
        assert (dec == dec[0]).all()
        got = [int(v) for v in dec[0]]
        assert all(min(a, b) <= g <= max(a, b) for g, a, b in zip(got, red_a, red_b)), got
        assert sum(abs(g - c) for g, c in zip(got, colour)) <= sum(abs(a - c) for a, c in zip(red_a, colour)), got
    y, x = np.mgrid[0:n, 0:n]
    ramp = np.stack([2 * x + 60, 2 * y + 40, x + y + 30, np.full_like(x, 255)], axis=-1).astype(np.uint8)
    dec = T.oracle_decode(T.PVRTC4, T.oracle_encode(T.PVRTC4, ramp, n, n, 4), n, n).reshape(n, n, 4)
    assert psnr(dec, ramp) > 30.0, psnr(dec, ramp)
    for gen in ("noise", "smooth", "flat", "mixed"):
        img = T.GENERATORS[gen](256, 256, 4, index=3)
        d4 = T.oracle_decode(T.PVRTC4, T.oracle_encode(T.PVRTC4, img, 256, 256, 4), 256, 256).reshape(256, 256, 4)
        d2 = T.oracle_decode(T.PVRTC2, T.oracle_encode(T.PVRTC2, img, 256, 256, 4), 256, 256).reshape(256, 256, 4)
        assert psnr(d4, img) > psnr(d2, img), gen


def test_decode_math_matches_oracle(emul):
    emul.emul_decode.restype = ctypes.c_int
    emul.emul_decode.argtypes = [T.ci, T.ci, T.u32, T.u32, T.u32, T.vp, T.vp]
    g = np.random.Generator(np.random.PCG64(11))
    for codec, comps in ((T.DXT1, 3), (T.DXT5, 4), (T.ETC1, 3)):
        for swap in ((0, 1) if codec != T.ETC1 else (0,)):
            for (h, w, pad) in [(64, 64, 0), (13, 7, 0), (9, 9, 5)]:
                n = T.oracle().ico_encoded_size(codec, h, w)
                for kind in ("encoded", "random"):
                    if kind == "encoded":
                        blocks = T.oracle_encode(codec, T.s_mixed(h, w, 4 if codec == T.DXT5 else 3, index=3), h, w,
                                                 4 if codec == T.DXT5 else 3, swap)
                    else:
                        blocks = g.integers(0, 256, size=n, dtype=np.uint8).tobytes()
                        # (ETC1: differential blocks whose base + delta leaves 0..31 included: etc_compressor.cc:198-273
                        #  defines them through Extend5Bit's masks and ClampTo8Bits)
                    want = T.oracle_decode(codec, blocks, h, w, swap=swap, pad=pad)
                    out = np.zeros(h * (w * comps + pad), np.uint8)
                    bb = np.frombuffer(blocks, np.uint8)
                    assert emul.emul_decode(codec, swap, h, w, pad, bb.ctypes.data, out.ctypes.data)
                    assert np.array_equal(out, want), (codec, swap, h, w, pad, kind)


def test_blockops_math_matches_oracle(emul):
    emul.emul_pad.restype = ctypes.c_int
    emul.emul_pad.argtypes = [T.ci, T.ci, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp]
    emul.emul_downsample.restype = ctypes.c_int
    emul.emul_downsample.argtypes = [T.ci, T.ci, T.u32, T.u32, T.vp, T.vp]
    emul.emul_transcode.restype = None
    emul.emul_transcode.argtypes = [T.vp, T.sz]
    for compressor, fmt, codec, strategy in [(T.DXTC, T.RGB, T.DXT1, 2), (T.DXTC, T.BGRA, T.DXT5, 2), (T.ETC, T.RGB, T.ETC1, 0),
                                            (T.ETC, T.RGB, T.ETC1, 2), (T.ETC, T.RGB, T.ETC1, 3)]:
        bb = 16 if codec == T.DXT5 else 8
        for (h, w) in [(32, 48), (13, 7), (64, 8), (8, 64), (4, 4), (2, 2), (1, 4), (4, 1), (3, 8), (16, 16)]:
            img = T.s_mixed(h, w, T.comps_of(fmt), index=h + w)
            blocks = T.oracle_compress(compressor, fmt, img, h, w, 0, strategy)
            b = np.frombuffer(blocks, np.uint8)
            ch, cw = 4 * ((h + 3) // 4), 4 * ((w + 3) // 4)
            for (ph, pw) in [(h + 9, w + 5), (ch, cw + 8), (ch + 4, cw)]:
                want = T.oracle_pad(compressor, fmt, blocks, ch, cw, ph, pw, strategy)
                out = np.zeros(((ph + 3) // 4) * ((pw + 3) // 4) * bb, np.uint8)
                assert emul.emul_pad(codec, strategy, ch, cw, ph, pw, b.ctypes.data, out.ctypes.data)
                assert out.tobytes() == want, (codec, h, w, ph, pw)
            want = T.oracle_downsample(compressor, fmt, blocks, h, w, strategy)
            out = np.zeros(max(len(want) if want else 0, bb), np.uint8)
            ok = emul.emul_downsample(codec, strategy, h, w, b.ctypes.data, out.ctypes.data)
            assert (out[:len(want)].tobytes() if ok else None) == want, (codec, h, w)
    # r05: Pad of ARBITRARY ETC1 block words with kSmallerError -- the border kernel's four-lanes-per-block search
    # (encode_etc1_block_quad; the emulation runs it next to the one-lane form and poisons the output on a difference) against
    # the oracle: saturated bases, clamping codewords, individual and differential blocks, ties between the partitions
    g = np.random.Generator(np.random.PCG64(29))
    for trial in range(8):
        h, w = 32, 64
        raw = g.integers(0, 256, size=(h // 4) * (w // 4) * 8, dtype=np.uint8)
        if trial >= 6:  # few distinct values: equal rows / columns, partition ties
            raw = (raw & (0xc0 if trial == 6 else 0x81)).astype(np.uint8)
        for (ph, pw) in [(h + 8, w + 8), (h, w + 4), (h + 4, w)]:
            want = T.oracle_pad(T.ETC, T.RGB, raw.tobytes(), h, w, ph, pw, 2)
            out = np.zeros((ph // 4) * (pw // 4) * 8, np.uint8)
            assert emul.emul_pad(T.ETC1, 2, h, w, ph, pw, raw.ctypes.data, out.ctypes.data)
            assert out.tobytes() == want, (trial, ph, pw)
    # Downsample of ARBITRARY block words (not encoder output): DXT1 three-colour mode and equal endpoints, DXT5 six-value
    # alpha -- the kernel's palette-plane / quad-selector form (dxt_downsample_2x2) against the oracle's decode-average-encode
    g = np.random.Generator(np.random.PCG64(17))
    for compressor, fmt, codec in [(T.DXTC, T.RGB, T.DXT1), (T.DXTC, T.RGBA, T.DXT5), (T.ETC, T.RGB, T.ETC1)]:
        bb = 16 if codec == T.DXT5 else 8
        for trial in range(6):  # (ETC1: random words = half differential, many with a base outside 0..31)
            h, w = 32, 64
            raw = g.integers(0, 256, size=(h // 4) * (w // 4) * bb, dtype=np.uint8).reshape(-1, bb)
            col = raw[:, bb - 8:]
            if trial == 1:   # c0 < c1 everywhere (DXT1: three colours + black)
                c = np.sort(col[:, :4].copy().view(np.uint16), axis=1)
                col[:, :4] = c.view(np.uint8)
            elif trial == 2:  # c0 == c1
                col[:, 2:4] = col[:, 0:2]
            elif trial == 3 and codec == T.DXT5:  # alpha0 <= alpha1: the six-value mode
                a = np.sort(raw[:, :2], axis=1)
                raw[:, :2] = a
            blocks = raw.tobytes()
            strategy = 3 if codec == T.ETC1 else 2
            want = T.oracle_downsample(compressor, fmt, blocks, h, w, strategy)
            out = np.zeros(len(want), np.uint8)
            b = np.frombuffer(blocks, np.uint8)
            assert emul.emul_downsample(codec, strategy, h, w, b.ctypes.data, out.ctypes.data), (codec, trial)
            assert out.tobytes() == want, (codec, trial)
    g = np.random.Generator(np.random.PCG64(3))
    raw = g.integers(0, 256, size=8 * 2048, dtype=np.uint8)
    want = T.oracle_transcode(raw.tobytes())
    emul.emul_transcode(raw.ctypes.data, raw.size)
    assert raw.tobytes() == want
    # the palette-domain transcoder (transcode_dxt1_block_to_etc1) on more kinds of blocks: 64 k random words, three-colour
    # mode (c0 < c1), equal endpoints, all-one-index blocks, and the encoder's own output for every synthetic content
    cases = [g.integers(0, 256, size=8 * 65536, dtype=np.uint8)]
    r = g.integers(0, 256, size=(8192, 8), dtype=np.uint8)
    r[:, :4] = np.sort(r[:, :4].copy().view(np.uint16), axis=1).view(np.uint8)
    cases.append(r.reshape(-1).copy())
    r = g.integers(0, 256, size=(8192, 8), dtype=np.uint8)
    r[:, 2:4] = r[:, 0:2]
    cases.append(r.reshape(-1).copy())
    r = g.integers(0, 256, size=(4096, 8), dtype=np.uint8)
    r[:, 4:] = np.repeat(np.array([0x00, 0x55, 0xaa, 0xff], np.uint8), 1024)[:, None]
    cases.append(r.reshape(-1).copy())
    for gen in ("noise", "smooth", "flat", "mixed"):
        cases.append(np.frombuffer(T.oracle_compress(T.DXTC, T.RGB, T.GENERATORS[gen](128, 128, 3, index=11), 128, 128), np.uint8).copy())
    for raw in cases:
        want = T.oracle_transcode(raw.tobytes())
        emul.emul_transcode(raw.ctypes.data, raw.size)
        assert raw.tobytes() == want


def test_random_soak_host_emulation(emul):
    """The GPU tier's soak (tests/test_gpu_parity.py) with the device math emulated on the host, smaller sizes."""
    n = 0
    for (codec, comps, swap, strategy, h, w, pad, img) in T.soak_cases(0x50AD, 120, 20, max_h=70, max_w=90,
                                                                      max_log2_pvrtc=3):
        src = T.with_row_padding(img, pad)
        stride = w * comps + pad
        want = T.oracle_encode(codec, src, h, w, comps, swap, strategy, stride=stride)
        assert emul_encode(emul, codec, src, h, w, comps, swap, strategy, stride=stride) == want, \
            (codec, comps, swap, strategy, h, w, pad)
        n += 1
    assert n == 140


def _alpha_blocks_exhaustive():
    """Alpha values of 4x4 blocks that drive ComputeAlphaBits (dxtc.cc:427-479) through every (alpha0, alpha1, alpha)
    it can see: 8-value mode = exactly one pixel each at the maximum and the minimum and every value in between;
    6-value mode = two zeros and / or two 255s next to a non-extreme range [lo, hi] and every value inside it."""
    rows = []
    for a0 in range(1, 256):            # 8-value mode: a0 > a1, the extremes appear once (incl. 0 and 255)
        for a1 in range(0, a0):
            inner = list(range(a1 + 1, a0))
            fill = (a0 + a1) // 2 if inner else (a0 if a0 < 255 else a1)
            if not inner and fill in (0, 255):
                continue                # (255, 254 .. 0): no non-extreme filler exists that keeps the mode
            for i in range(0, max(len(inner), 1), 14):
                rows.append(([a0, a1] + inner[i:i + 14] + [fill] * 14)[:16])
    for lo in range(1, 255):            # 6-value mode: a0 = lo <= a1 = hi, specials 0 / 255 present
        for hi in range(lo, 255):
            inner = list(range(lo, hi + 1))
            for specials in ([0, 0], [255, 255], [0, 0, 255], [0, 255, 255]):
                room = 16 - len(specials) - 2
                for i in range(0, len(inner), room):
                    rows.append(([lo, hi] + specials + inner[i:i + room] + [lo] * room)[:16])
    for v in range(256):                # all equal; only extremes (the (0, 255) reset, dxtc.cc:400-403)
        rows.append([v] * 16)
        rows.append([0] * (v % 15 + 1) + [255] * (15 - v % 15))
    return np.asarray(rows, np.uint8)


def test_dxt5_alpha_index_search_exhaustive(emul):
    """The O(1) alpha index search (dxt_block.h + the generated dxt5_alpha_index_table.inc) against the oracle's
    8-candidate scan for every (alpha0, alpha1, alpha) of both modes -- about 1.3 M blocks."""
    alphas = _alpha_blocks_exhaustive()
    g = np.random.Generator(np.random.PCG64(5))
    n = alphas.shape[0]
    perm = np.argsort(g.random((n, 16)), axis=1)          # shuffle pixel positions inside each block
    alphas = np.take_along_axis(alphas, perm, axis=1)
    chunk = 1 << 16
    for s in range(0, n, chunk):
        a = alphas[s:s + chunk]
        m = a.shape[0]
        img = np.zeros((4, 4 * m, 4), np.uint8)
        img[..., :3] = g.integers(0, 256, (4, 4 * m, 3), dtype=np.uint8)
        img[..., 3] = a.reshape(m, 4, 4).transpose(1, 0, 2).reshape(4, 4 * m)
        want = T.oracle_encode(T.DXT5, img, 4, 4 * m, 4)
        got = emul_encode(emul, T.DXT5, img, 4, 4 * m, 4)
        if got != want:
            w_ = np.frombuffer(want, np.uint8).reshape(m, 16)[:, :8]
            g_ = np.frombuffer(got, np.uint8).reshape(m, 16)[:, :8]
            bad = np.nonzero((w_ != g_).any(axis=1))[0][:5]
            raise AssertionError([(a[i].tolist(), w_[i].tolist(), g_[i].tolist()) for i in bad])


def _pvrtc_random_words(g, n_blocks):
    """Random PVRTC block words (any bit pattern decodes; both block kinds and all sub-modes occur)."""
    return g.integers(0, 256, size=8 * n_blocks, dtype=np.uint8)


def test_pvrtc_decode_math_matches_oracle(emul):
    """PVRTC 2bpp decoder (extension, parity unpinned -- the reference has none): device block math vs the oracle's
    plain-C statement of the same rules, on encoder output and on random block words."""
    emul.emul_decode.restype = ctypes.c_int
    emul.emul_decode.argtypes = [T.ci, T.ci, T.u32, T.u32, T.u32, T.vp, T.vp]
    g = np.random.Generator(np.random.PCG64(23))
    for n in (8, 16, 64, 128):
        cases = [np.frombuffer(T.oracle_encode(T.PVRTC2, T.GENERATORS[gen](n, n, 4, index=n), n, n, 4), np.uint8)
                 for gen in ("noise", "smooth", "flat", "mixed")]
        cases.append(_pvrtc_random_words(g, n * n // 32))
        for blocks in cases:
            want = T.oracle_decode(T.PVRTC2, blocks.tobytes(), n, n)
            out = np.zeros(n * n * 4, np.uint8)
            b = np.ascontiguousarray(blocks)
            assert emul.emul_decode(T.PVRTC2, 0, n, n, 0, b.ctypes.data, out.ctypes.data)
            assert np.array_equal(out, want), n


def test_pvrtc4_decode_math_matches_oracle(emul):
    """PVRTC 4 bpp decoder (r05; extension of an extension, parity unpinned): device block math vs the oracle's plain-C
    statement of the same rules, on the 4 bpp encoder's output and on random block words -- half of which carry the
    punch-through flag the encoder never writes (weights 0, 4, 4, 8, alpha 0 for value 2)."""
    emul.emul_decode.restype = ctypes.c_int
    emul.emul_decode.argtypes = [T.ci, T.ci, T.u32, T.u32, T.u32, T.vp, T.vp]
    g = np.random.Generator(np.random.PCG64(31))
    for n in (8, 16, 64, 128):
        cases = [np.frombuffer(T.oracle_encode(T.PVRTC4, T.GENERATORS[gen](n, n, 4, index=n), n, n, 4), np.uint8)
                 for gen in ("noise", "smooth", "flat", "mixed")]
        cases += [g.integers(0, 256, size=n * n // 2, dtype=np.uint8) for _ in range(3)]
        for blocks in cases:
            want = T.oracle_decode(T.PVRTC4, blocks.tobytes(), n, n)
            out = np.zeros(n * n * 4, np.uint8)
            b = np.ascontiguousarray(blocks)
            assert emul.emul_decode(T.PVRTC4, 0, n, n, 0, b.ctypes.data, out.ctypes.data)
            assert np.array_equal(out, want), n


def test_pvrtc_decode_properties():
    """What ties the (reference-less) PVRTC decoder to the ENCODER's model: a solid texture decodes to the encoder's
    channel-reduced colour (pvrtc.cc:337-349); in a 1BPP block the block-centre pixels (x % 8 == 4, y % 4 == 2), where
    the up-sampling is the identity (pvrtc.cc:216-227), are exactly the stored colour A or B; and decoding a smooth
    opaque texture gives a sane PSNR."""
    for colour, want in (((200, 100, 50, 255), {(206, 99, 50, 255), (206, 99, 51, 255)}),   # R5 G5 B4 / B5
                         ((200, 100, 50, 100), {(204, 102, 36, 109), (204, 102, 51, 109)})):  # R4 G4 B3 / B4, A3
        img = np.zeros((32, 32, 4), np.uint8)
        img[...] = colour
        dec = T.oracle_decode(T.PVRTC2, T.oracle_encode(T.PVRTC2, img, 32, 32, 4), 32, 32).reshape(-1, 4)
        assert set(map(tuple, dec.tolist())) <= want, set(map(tuple, dec.tolist()))

    def rep(v, bits):
        e = v << (8 - bits)
        return e | e >> bits | (e >> 2 * bits if bits <= 3 else 0)
    n = 64
    img = T.s_flat(n, n, 4, index=4)
    blocks = np.frombuffer(T.oracle_encode(T.PVRTC2, img, n, n, 4), np.uint8).reshape(-1, 8)
    dec = T.oracle_decode(T.PVRTC2, blocks.tobytes(), n, n).reshape(n, n, 4)
    checked = 0
    for by in range(n // 4):
        for bx in range(n // 8):
            z = 0
            for i in range(16):
                z |= ((by >> i) & 1) << (2 * i) | ((bx >> i) & 1) << (2 * i + 1)
            data = int.from_bytes(blocks[z, :4].tobytes(), "little")
            cw = int.from_bytes(blocks[z, 4:].tobytes(), "little")
            if cw & 1:
                continue  # 2BPP block
            if (data >> (8 * 2 + 4)) & 1:  # pixel (4, 2) uses colour B
                c = (rep(cw >> 26 & 31, 5), rep(cw >> 21 & 31, 5), rep(cw >> 16 & 31, 5), 255) if cw >> 31 else \
                    (rep(cw >> 24 & 15, 4), rep(cw >> 20 & 15, 4), rep(cw >> 16 & 15, 4), rep(cw >> 28 & 7, 3))
            else:
                c = (rep(cw >> 10 & 31, 5), rep(cw >> 5 & 31, 5), rep(cw >> 1 & 15, 4), 255) if cw >> 15 & 1 else \
                    (rep(cw >> 8 & 15, 4), rep(cw >> 4 & 15, 4), rep(cw >> 1 & 7, 3), rep(cw >> 12 & 7, 3))
            assert tuple(dec[by * 4 + 2, bx * 8 + 4].tolist()) == c, (bx, by)
            checked += 1
    assert checked > 20
    y, x = np.mgrid[0:256, 0:256]
    img = np.zeros((256, 256, 4), np.uint8)
    img[..., 0] = (128 + 100 * np.sin(x / 40.0)).astype(np.uint8)
    img[..., 1] = (128 + 100 * np.cos(y / 33.0)).astype(np.uint8)
    img[..., 2] = ((x + y) // 2).astype(np.uint8)
    img[..., 3] = 255
    dec = T.oracle_decode(T.PVRTC2, T.oracle_encode(T.PVRTC2, img, 256, 256, 4), 256, 256).reshape(256, 256, 4)
    mse = ((dec.astype(np.float64) - img) ** 2).mean()
    assert 10 * np.log10(255 * 255 / mse) > 30.0


def constant_block_strip(colours, comps, alpha=None):
    """One 4x4 block per colour, every pixel of a block that colour (alpha, if any, varies inside the block: ignored)."""
    n = len(colours)
    px = np.repeat(np.asarray(colours, np.uint8).reshape(n, 1, 3), 16, axis=1)
    if comps == 4:
        a = np.arange(n * 16, dtype=np.uint32).reshape(n, 16, 1) * 37 if alpha is None else alpha
        px = np.concatenate([px, (a & 255).astype(np.uint8)], axis=2)
    return np.ascontiguousarray(px.reshape(n, 4, 4, comps).transpose(1, 0, 2, 3).reshape(4, 4 * n, comps))


def test_etc1_one_colour_blocks(emul):
    """The one-colour form of the ETC1 encoder (encode_etc1_constant_block: one pixel against the 32 candidates instead
    of four searches) against the oracle's full search (etc.cc:545-586): every grey level, every value of one channel
    against dark / bright others, the colours next to every 5-bit step, and 2^19 random colours; all three searching
    strategies, RGB and RGBA (alpha ignored) sources.  The GPU tier sweeps all 2^24 colours."""
    g = np.random.Generator(np.random.PCG64(2024))
    cols = [(v, v, v) for v in range(256)]
    for ch in range(3):
        for other in (0, 7, 8, 128, 247, 248, 255):
            for v in range(256):
                c = [other] * 3
                c[ch] = v
                cols.append(tuple(c))
    cols += [tuple(int(x) for x in r) for r in g.integers(0, 256, size=(1 << 19, 3))]
    cols = np.array(cols, np.uint8)
    n = len(cols)
    for comps, strategy in ((3, 2), (3, 0), (3, 1), (4, 2)):
        strip = constant_block_strip(cols, comps)
        want = T.oracle_encode(T.ETC1, strip, 4, 4 * n, comps, 0, strategy)
        got = emul_encode(emul, T.ETC1, strip, 4, 4 * n, comps, 0, strategy)
        if got != want:
            bad = [i for i in range(n) if got[i * 8:(i + 1) * 8] != want[i * 8:(i + 1) * 8]]
            raise AssertionError((comps, strategy, len(bad), [tuple(cols[i]) for i in bad[:5]]))
        # ... and the general forms agree on the same blocks (the kernel takes them when a wave is not all one-colour)
        assert emul_encode(emul, T.ETC1, strip[:, :4 * 4096], 4, 4 * 4096, comps, 0, strategy | 0x200) == want[:8 * 4096]


def etc_shortcut_blocks(g, n, comps):
    """n 4x4 blocks (4 x 4n strip) aimed at the unclamped shortcut of etc1_block.h: mid-tone base colours (so that the
    shortcut applies up to some codeword) with per-pixel deviations drawn around the decision points 2|s| = 3 (a + b)
    of every codeword (s = pixel sum - base sum), plus plain jitter of several amplitudes."""
    base = g.integers(40, 216, size=(n, 1, 3), dtype=np.int64)
    thr = np.array([15, 33, 57, 82, 117, 156, 208, 345])[g.integers(0, 8, size=(n, 16, 1))]  # 3 (a + b) / 2
    sign = g.choice(np.array([-1, 1]), size=(n, 16, 1))
    mode = g.integers(0, 3, size=(n, 1, 1))
    near = sign * (thr + g.integers(-2, 3, size=(n, 16, 1)))          # pixel sum deviation near a threshold
    split = g.integers(0, 3, size=(n, 16, 1))
    dev = np.zeros((n, 16, 3), np.int64)
    for c in range(3):                                                 # spread the deviation over the channels
        dev[:, :, c:c + 1] = near // 3 + (split == c) * (near - 3 * (near // 3))
    jitter = g.integers(-1, 2, size=(n, 16, 3)) * np.array([1, 4, 24])[g.integers(0, 3, size=(n, 1, 1))]
    px = np.where(mode == 0, base + dev, np.where(mode == 1, base + jitter, base + dev + jitter))
    px = np.clip(px, 0, 255).astype(np.uint8)
    if comps == 4:
        px = np.concatenate([px, g.integers(0, 256, size=(n, 16, 1), dtype=np.uint8)], axis=2)
    return np.ascontiguousarray(px.reshape(n, 4, 4, comps).transpose(1, 0, 2, 3).reshape(4, 4 * n, comps))


def test_etc1_unclamped_shortcut_on_decision_points(emul):
    """The sum form of the ETC1 unclamped shortcut (one v_sad per pixel and codeword, winner's modifiers worked out
    afterwards; r03) against the oracle's exhaustive scan (etc.cc:350-409), all search strategies."""
    g = np.random.Generator(np.random.PCG64(404))
    n = 1 << 15
    for comps, strategy in ((3, 2), (3, 0), (3, 1), (4, 2)):
        strip = etc_shortcut_blocks(g, n, comps)
        want = T.oracle_encode(T.ETC1, strip, 4, 4 * n, comps, 0, strategy)
        for force in (0, 0x100, 0x200, 0x400):  # as in the kernel / busy form everywhere / calm form everywhere / plain form
            got = emul_encode(emul, T.ETC1, strip, 4, 4 * n, comps, 0, strategy | force)
            if got != want:
                bad = [i for i in range(n) if got[i * 8:(i + 1) * 8] != want[i * 8:(i + 1) * 8]]
                raise AssertionError((comps, strategy, force, len(bad), bad[:5]))
    # the mixed tier on plain random and saturated content as well
    strip = g.integers(0, 256, size=(4, 4 * n, 3), dtype=np.uint8)
    strip[:, : n] = g.choice(np.array([0, 3, 40, 128, 215, 252, 255], np.uint8), size=(4, n, 3))
    for strategy in (0, 1, 2):
        want = T.oracle_encode(T.ETC1, strip, 4, 4 * n, 3, 0, strategy)
        for force in (0x100, 0x200, 0x400):
            assert emul_encode(emul, T.ETC1, strip, 4, 4 * n, 3, 0, strategy | force) == want, (strategy, force)
