"""CPU tier for BC7 (include/ic_amd.h ICAMD_BC7).

* The decoder: the numpy restatement (tests/bc7_oracle.py) and the host twin of csrc/bc7_block.h (tests/host_emul/bc7_emul.cc,
  -DICAMD_HOST_EMULATION) against the committed fixture (tests/golden/bc7_decode_kat.bin: texels of an independent decoder),
  the twin against the restatement on 4096 further blocks, every table entry probed through Pillow.
* The mode-6 encoder: the twin bit-exact against the definition's restatement on every shape, layout and content, hand-built
  blocks for every branch, the invariants of the written blocks, the quality conditions on the oracle alone.
* The metric's twin against numpy.
* The C ABI's host-side surface: ids, sizes, kernel names, statuses, refusals, container framing, the prototype table.
* The new kernels compile without scratch."""
import ctypes
import functools
import importlib
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bc7_oracle as B
import ic_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
KAT = os.path.join(HERE, "golden", "bc7_decode_kat.bin")
pkg = importlib.import_module("image-compression_amd")
BC7 = B.BC7
SHAPES = [(1, 1), (4, 4), (5, 3), (9, 2), (61, 59)]
PAD = 6  # bytes of row padding
PADDED = [(5, 3, 16, 16), (30, 30, 40, 48)]
U64P = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bc7") / "libbc7_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC,
                           "-I" + os.path.join(T.ROOT, "include"), "-o", so, os.path.join(EMUL_DIR, "bc7_emul.cc")])
    L = ctypes.CDLL(so)
    L.bc7_emul_encode.restype = ctypes.c_int
    L.bc7_emul_encode.argtypes = [T.ci, T.ci, T.u32, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp]
    L.bc7_emul_decode.restype = ctypes.c_int
    L.bc7_emul_decode.argtypes = [T.ci, T.u32, T.u32, T.u32, T.vp, T.vp]
    L.bc7_emul_metric.restype = ctypes.c_int
    L.bc7_emul_metric.argtypes = [T.ci, T.ci, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp, U64P]
    yield L
    T.assert_no_emul_violations(L, "test_bc7_host")


def emul_encode(L, img, gh=None, gw=None, swap=False, pad=0):
    h, w, comps = img.shape
    out = np.zeros(B.encoded_size(max(h, gh or h), max(w, gw or w)), np.uint8)
    src = np.ascontiguousarray(T.with_row_padding(img, pad) if pad else img).reshape(-1)
    assert L.bc7_emul_encode(comps, int(swap), h, w, gh or h, gw or w, w * comps + pad, src.ctypes.data, out.ctypes.data)
    return out.tobytes()


def emul_decode(L, blocks, h, w, pad=0, swap=False):
    out = np.zeros((h, w * 4 + pad), np.uint8)
    b = np.frombuffer(bytes(blocks), np.uint8).copy()
    assert L.bc7_emul_decode(int(swap), h, w, pad, b.ctypes.data, out.ctypes.data)
    return out


def encode_texels_emul(L, v):
    """[N, 16, 4] texels (R, G, B, A) as N blocks of a 4-row RGBA8 image through the twin -> [N, 16] uint8."""
    n = len(v)
    img = np.asarray(v, np.uint8).reshape(n, 4, 4, 4).transpose(1, 0, 2, 3).reshape(4, 4 * n, 4)
    return np.frombuffer(emul_encode(L, np.ascontiguousarray(img)), np.uint8).reshape(n, 16)


@functools.lru_cache(maxsize=None)
def kat():
    rec = np.fromfile(KAT, np.uint8).reshape(-1, 80)
    assert rec.shape[0] == 600
    rec.setflags(write=False)
    return rec[:, :16], rec[:, 16:].reshape(-1, 16, 4)


def kat_rows(want):
    """[n, 16, 4] texels -> the [4, n * 16] RGBA8 rows of the blocks laid out as a 4-row image."""
    n = len(want)
    return want.reshape(n, 4, 4, 4).transpose(1, 0, 2, 3).reshape(4, n * 16)


# ---- decoder

def test_fixture_holds_every_cell_the_generator_promises():
    blocks, want = kat()
    modes = [(int(b[0]) & -int(b[0])).bit_length() - 1 for b in blocks]  # -1: byte 0 is 0, the reserved form
    assert [modes.count(m) for m in range(8)] == [33, 129, 129, 129, 9, 5, 33, 129] and modes.count(-1) == 4
    for m in (0, 1, 2, 3, 7):
        pb = B.MODES[m][1]
        parts = [(int.from_bytes(bytes(b), "little") >> (m + 1)) & ((1 << pb) - 1) for b, mm in zip(blocks, modes) if mm == m]
        assert all(parts.count(p) >= 2 for p in range(1 << pb)), m
    assert not want[-4:].any() and all(b[0] == 0 and b[1:].any() for b in blocks[-4:])  # reserved: zeros by the specification


def test_oracle_decode_equals_the_fixture():
    blocks, want = kat()
    assert (B.decode_blocks(blocks.tobytes()) == want).all()


def test_twin_decode_equals_the_fixture(emul):
    blocks, want = kat()
    got = emul_decode(emul, blocks.tobytes(), 4, 4 * len(blocks))
    assert (got == kat_rows(want)).all()
    swapped = emul_decode(emul, blocks.tobytes(), 4, 4 * len(blocks), swap=True)
    assert (swapped.reshape(4, -1, 4) == got.reshape(4, -1, 4)[..., [2, 1, 0, 3]]).all()


def test_twin_decode_equals_the_oracle_on_4096_stratified_blocks(emul):
    blocks = B.stratified_blocks(4096, seed=7001)
    assert (emul_decode(emul, blocks, 4, 4 * 4096) == B.decode(blocks, 4, 4 * 4096)).all()


def test_twin_decode_padded_rows_and_clipped_shapes(emul):
    for i, (h, w) in enumerate(SHAPES):
        blocks = B.stratified_blocks(B.encoded_size(h, w) // 16, seed=7100 + i)
        assert (emul_decode(emul, blocks, h, w, PAD) == B.decode(blocks, h, w, PAD)).all(), (h, w)


def test_every_table_entry_against_pillow():
    """Partition entries: a block with a distinct flat colour per subset and every index 0 shows each texel's subset.  Anchor
    entries: endpoints (0, 255) in every subset and every index bit one -- the texels that do not decode to the top are the
    ones whose index has one bit fewer."""
    pytest.importorskip("PIL")
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_bc7_golden as G
    # mode 2 (three subsets, 6 partition bits, 5-bit colours, no p-bits) and mode 3 (two subsets, 7-bit colours + p-bits)
    blocks = []
    for part in range(64):
        v = 1 << 2 | part << 3  # mode 2: R of the six endpoints at bit 9, 5 bits each
        for e, r in enumerate((4, 4, 12, 12, 20, 20)):
            v |= r << (9 + 5 * e)
        blocks.append(v.to_bytes(16, "little"))
    for part in range(64):
        v = 1 << 3 | part << 4  # mode 3: R of the four endpoints at bit 10, 7 bits each
        for e, r in enumerate((16, 16, 80, 80)):
            v |= r << (10 + 7 * e)
        blocks.append(v.to_bytes(16, "little"))
    dec = G.pillow_decode(b"".join(blocks))
    red3 = dec[:64, :, 0]
    assert (np.searchsorted([33, 99, 165], red3) == B.P3).all()  # 4, 12, 20 expand to 33, 99, 165
    red2 = dec[64:, :, 0]
    assert np.isin(red2, (32, 160)).all() and ((red2 == 160) == B.P2).all()  # 16, 80 with p = 0 are 32, 160
    assert np.isin(red3, (33, 99, 165)).all()
    # anchors: endpoints (0, 255) in every subset, indices all ones.  A texel with the full index width decodes to 255; the
    # anchor of a subset reads one bit fewer, so every texel after it reads its bits one position early -- still all ones --
    # and the anchor itself decodes to the weight of the all-ones index of width - 1.  Mode 3 (2-bit indices): an anchor reads
    # index 1 (weight 21 -> 84), the others 3 (255).  Mode 2 likewise.
    blocks = []
    for part in range(64):
        v = ((1 << 128) - 1) >> 99 << 99 | 1 << 2 | part << 3  # mode 2: indices from bit 99 all ones
        for c in range(3):
            for e in (1, 3, 5):
                v |= 31 << (9 + 30 * c + 5 * e)
        blocks.append(v.to_bytes(16, "little"))
    for part in range(64):
        v = ((1 << 128) - 1) >> 98 << 98 | 1 << 3 | part << 4  # mode 3: indices from bit 98 all ones; p-bits 94..97 stay 0
        for c in range(3):
            for e in (1, 3):
                v |= 127 << (10 + 28 * c + 7 * e)
        blocks.append(v.to_bytes(16, "little"))
    dec = G.pillow_decode(b"".join(blocks))
    for part in range(64):
        low3 = sorted(np.flatnonzero(dec[part, :, 0] != 255).tolist())
        assert low3 == sorted({0, int(B.A3A[part]), int(B.A3B[part])}), part
        low2 = sorted(np.flatnonzero(dec[64 + part, :, 0] < 250).tolist())
        assert low2 == sorted({0, int(B.A2[part])}), part
        assert [B.subset_of(3, part, a) for a in B.anchors(3, part)] == [0, 1, 2]
        assert [B.subset_of(2, part, a) for a in B.anchors(2, part)] == [0, 1]


# ---- encoder against the definition

@functools.lru_cache(maxsize=None)
def _image(name, h, w, comps):
    img = B.content(name, h, w, comps, seed=len(name))
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _want(name, h, w, comps, gh=None, gw=None, swap=False):
    return B.oracle_encode(_image(name, h, w, comps), gh, gw, swap)


@pytest.mark.parametrize("comps", [3, 4])
@pytest.mark.parametrize("swap", [False, True])
def test_encoder_matches_definition_on_every_shape(emul, comps, swap):
    for h, w in SHAPES:
        img = _image("noise", h, w, comps)
        assert emul_encode(emul, img, swap=swap, pad=PAD) == _want("noise", h, w, comps, swap=swap), (h, w)


@pytest.mark.parametrize("name", B.CONTENTS)
def test_encoder_matches_definition_on_every_content(emul, name):
    for comps in (3, 4):
        img = _image(name, 61, 59, comps)
        assert emul_encode(emul, img) == _want(name, 61, 59, comps), comps


@pytest.mark.parametrize("h,w,gh,gw", PADDED)
def test_encoder_padded_grid(emul, h, w, gh, gw):
    for comps, swap in ((3, False), (4, True)):
        img = _image("smooth", h, w, comps)
        assert emul_encode(emul, img, gh=gh, gw=gw, swap=swap) == _want("smooth", h, w, comps, gh, gw, swap)


def _blk(f):
    return np.array([f(i) for i in range(16)], np.int64)


def test_hand_built_blocks_force_every_branch(emul):
    grey = lambda g: (g, g, g, 255)  # noqa: E731
    v = np.stack([
        _blk(lambda i: (10, 20, 30, 255)),                                            # 0 flat: det = 0
        _blk(lambda i: (10, 20, 30, 254) if i % 2 else (200, 100, 50, 254)),            # 1 refit rejected (first pass exact)
        _blk(lambda i: grey(100 + 2 * i) if i != 5 else grey(255)),                     # 2 refit accepted (an outlier)
        _blk(lambda i: grey(240 - 16 * i)),                                             # 3 anchor flip: texel 0 the brightest
        _blk(lambda i: (10, 21, 30, 41)),                                               # 4 p-bit tie: err(0) = err(1) = 2
        _blk(lambda i: (0, 1, 1, 1)),                                                   # 5 T = 0 with p = 1
        _blk(lambda i: (255, 0, 0, 0)),                                                 # 6 T = 255 with p = 0
        _blk(lambda i: (16 * i, 240 - 16 * i, 0, 255)),                                 # 7 negative covariance
        _blk(lambda i: (100, 100, 100, 16 * i)),                                        # 8 c* = A
    ])
    blocks, sse1, final, take = B.encode_texels(v, stages=True)
    t0, t1 = B.targets(v)
    k, _ = B.indices(v, B.quantise(t0), B.quantise(t1))
    _, _, has_refit = B.refit_targets(v, k)
    # the branches are the ones named
    assert not has_refit[0] and has_refit[1:4].all()
    assert sse1[1] == 0 and not take[1] and final[1] == 0
    assert take[2] and final[2] < sse1[2]
    assert k[3, 0] >= 8 and k[0, 0] < 8
    assert (B.quantise(np.array([[10, 21, 30, 41]])) == [[10, 22, 30, 42]]).all() and blocks[4, 7] >> 7 == 0  # the tie takes p = 0
    assert (B.quantise(np.array([[0, 1, 1, 1]])) == [[1, 1, 1, 1]]).all()
    assert (B.quantise(np.array([[255, 0, 0, 0]])) == [[254, 0, 0, 0]]).all()
    assert t0[7].tolist() == [0, 240, 0, 255] and t1[7].tolist() == [240, 0, 0, 255]
    assert t0[8].tolist() == [100, 100, 100, 0] and t1[8].tolist() == [100, 100, 100, 240]
    assert blocks[0].tobytes().hex() == "c04241a1783cfe7f" + "00" * 8  # the header's example
    # the twin writes the definition's blocks
    assert (encode_texels_emul(emul, v) == blocks).all()
    # every 4-channel tie order of c*: R before G before B before A
    ties = np.stack([_blk(lambda i, c=c: tuple(16 * i if ch >= c else 7 for ch in range(4))) for c in range(4)])
    tt0, tt1 = B.targets(ties)
    assert (tt0 <= tt1).all()  # positive covariance with the first widest channel: nothing exchanged
    assert (encode_texels_emul(emul, ties) == B.encode_texels(ties)).all()


def test_written_blocks_are_mode_6_with_a_clear_anchor_bit_and_decode_alike_both_ways(emul):
    img = _image("noise", 61, 59, 4)
    blocks = np.frombuffer(emul_encode(emul, img), np.uint8).reshape(-1, 16)
    assert (blocks[:, 0] & 0x7f == 0x40).all()  # bits 0..5 clear, bit 6 set
    # texel 0's index has 3 stored bits (65..67); its fourth, the anchor's MSB, is implied 0 -- the round trip at the end of
    # this test holds only if every k_0 the encoder meant was below 8.  The flipped form decodes alike:
    v = B.block_texels(img)
    t0, t1 = B.targets(v)
    e0, e1 = B.quantise(t0), B.quantise(t1)
    k, _ = B.indices(v, e0, e1)
    pal = lambda a, b, kk: ((64 - B.W4[kk])[..., None] * a[:, None, :] + B.W4[kk][..., None] * b[:, None, :] + 32) >> 6  # noqa: E731
    assert (pal(e0, e1, k) == pal(e1, e0, 15 - k)).all()
    # and the decoder reads what the encoder meant: the decoded texels are the palette entries the definition chose
    full, _, final, _ = B.encode_texels(v, stages=True)
    dec = B.decode_blocks(full.tobytes()).astype(np.int64)
    assert (((dec - v) ** 2).sum(axis=(1, 2)) == final).all()
    assert (full == blocks).all()


def test_refit_never_raises_a_blocks_error():
    for name in B.CONTENTS:
        _, sse1, final, take = B.encode_texels(B.block_texels(_image(name, 61, 59, 4)), stages=True)
        assert (final <= sse1).all() and (final[take] < sse1[take]).all() and (final[~take] == sse1[~take]).all(), name


def test_quality_against_the_dxt5_oracle():
    """Summed RGBA squared error over a 64 x 64 image, BC7 mode 6 (the definition) against the oracle's DXT5 encoder.
    Measured: ramp 114542 against 121453, smooth 318750 against 670688."""
    for name in ("ramp", "smooth"):
        img = B.content(name, 64, 64, 4)
        bc7 = B.sse_of(img, B.oracle_encode(img))
        dxt5 = T.oracle_decode(T.DXT5, T.oracle_encode(T.DXT5, img, 64, 64, 4), 64, 64).reshape(64, 64, 4).astype(np.int64)
        dxt5 = int(((dxt5 - img.astype(np.int64)) ** 2).sum())
        print(name, "bc7", bc7, "dxt5", dxt5)
        assert bc7 < dxt5, name


# ---- metric twin

@pytest.mark.parametrize("comps,swap", [(3, False), (4, False), (4, True)])
def test_metric_twin_matches_numpy(emul, comps, swap):
    h, w, gw = 30, 30, 48
    img = _image("smooth", h, w, comps)
    blocks = np.frombuffer(B.stratified_blocks(8 * 12, seed=7200), np.uint8).copy()  # every mode, a grid 48 wide
    out = (ctypes.c_uint64 * 8)()
    src = np.ascontiguousarray(img).reshape(-1)
    assert emul.bc7_emul_metric(comps, int(swap), h, w, gw, w * comps, src.ctypes.data, blocks.ctypes.data, out)
    own = blocks.reshape(8, 12, 16)[:, :8].tobytes()
    dec = B.decode(own, h, w, swap=swap).reshape(h, w, 4)[..., :comps].astype(np.int64)
    d = dec - img.astype(np.int64)
    want = list((d * d).sum(axis=(0, 1))) + [0] * (4 - comps) + list(np.abs(d).max(axis=(0, 1))) + [0] * (4 - comps)
    assert list(out) == want


# ---- the C ABI's host-side surface (no device work: every check below returns before the GPU is touched)

def test_codec_value_sizes_and_kernel_names():
    assert pkg.BC7 == 32 == BC7
    assert pkg.encoded_size(BC7, 8, 8) == 64 and pkg.encoded_size(BC7, 5, 3) == 32 and pkg.encoded_size(BC7, 257, 1023) == 65 * 256 * 16
    for comps in range(0, 6):
        assert pkg.kernel_name(BC7, comps) == {3: "icamd_bc7_rgb888_kernel", 4: "icamd_bc7_rgba8_kernel"}.get(comps, "")
        assert pkg.metric_kernel_name(BC7, comps) == {3: "icamd_metric_bc7_rgb888_kernel", 4: "icamd_metric_bc7_rgba8_kernel"}.get(comps, "")
    for codec in (26, 27, 28, 29, 30, 31, 33):
        for comps in (1, 2, 3, 4):
            assert pkg.kernel_name(codec, comps) == "" and pkg.metric_kernel_name(codec, comps) == ""
        assert pkg.container_size(pkg.CONTAINER_KTX, codec, 8, 8, 1) == 0


def test_encode_statuses():
    lib = pkg.lib()
    enc = lib.icamd_encode_device
    d = ctypes.c_void_p(16)  # never dereferenced: the arguments are refused first
    for comps in (0, 1, 2, 5):
        assert enc(BC7, 2, comps, 0, 8, 8, 8, 8, 64, 1, 0, 0, d, d, None) == -4, comps  # bad components
        assert b"src_components" in lib.icamd_last_error()
    for comps in (3, 4):
        assert enc(BC7, 2, comps, 0, 0, 8, 8, 8, 64, 1, 0, 0, d, d, None) == 1        # empty image
        assert enc(BC7, 2, comps, 0, 8, 0, 8, 8, 64, 1, 0, 0, d, d, None) == 1
        assert enc(BC7, 2, comps, 0, 8, 8, 8, 8, 64, 1, 0, 0, None, d, None) == 1     # null source
        assert enc(BC7, 2, comps, 0, 8, 8, 8, 8, 64, 1, 0, 0, d, None, None) == 1     # null output
        assert enc(BC7, 2, comps, 0, 8, 8, 8, 8, 64, 0, 0, 0, d, d, None) == 0        # no images
    # the statuses DXT5 gives for the same arguments, wherever no device is needed to answer
    for args in ((2, 9, 0, 0, 8, 8, 8, 64, 1), (2, 4, 0, 8, 8, 8, 8, 64, 0), (7, 4, 1, 8, 8, 8, 8, 64, 0)):
        assert enc(BC7, *args, 0, 0, d, d, None) == enc(pkg.DXT5, *args, 0, 0, d, d, None), args


def test_decode_and_measure_statuses():
    lib = pkg.lib()
    dec, met = lib.icamd_decode_device, lib.icamd_measure_error_device
    d = ctypes.c_void_p(16)
    assert dec(BC7, 0, 0, 8, 0, 1, 0, 0, d, d, None) == 1
    assert dec(BC7, 0, 8, 0, 0, 1, 0, 0, d, d, None) == 1
    assert dec(BC7, 0, 8, 8, 0, 1, 0, 0, None, d, None) == 1
    assert dec(BC7, 0, 8, 8, 0, 1, 0, 0, d, None, None) == 1
    assert dec(BC7, 1, 8, 8, 6, 0, 0, 0, d, d, None) == 0
    for comps in range(0, 6):
        want = 0 if comps in (3, 4) else -4
        assert met(BC7, comps, 0, 8, 8, 8, 8, 8 * max(comps, 1), 0, 0, 0, d, d, d, None) == want, comps
    for comps in (3, 4):
        assert met(BC7, comps, 0, 0, 8, 8, 8, 8 * comps, 1, 0, 0, d, d, d, None) == 1
        assert met(BC7, comps, 0, 8, 8, 8, 8, 8 * comps, 1, 0, 0, None, d, d, None) == 1
        assert met(BC7, comps, 0, 8, 8, 8, 8, 8 * comps, 1, 0, 0, d, None, d, None) == 1
        assert met(BC7, comps, 0, 8, 8, 8, 8, 8 * comps, 1, 0, 0, d, d, None, None) == 1
        assert met(BC7, comps, 1, 8, 8, 8, 8, 8 * comps, 0, 0, 0, d, d, d, None) == 0
        assert met(BC7, comps, 0, 8, 8, 8, 8, 8 * comps - 1, 0, 0, 0, d, d, d, None) == -4   # stride < row
        assert b"row stride" in lib.icamd_last_error()
        assert met(BC7, comps, 0, 8, 8, 4, 8, 8 * comps, 0, 0, 0, d, d, d, None) == -4       # grid < image
        assert met(BC7, comps, 0, 8, 8, 8, 4, 8 * comps, 0, 0, 0, d, d, d, None) == -4
        assert b"grid" in lib.icamd_last_error()
        assert met(BC7, comps, 0, 8, 8, 8, 8, 8 * comps, 0, 0, 0, d, d, ctypes.c_void_p(20), None) == -4  # d_stats alignment


def test_the_other_entry_points_refuse_bc7_as_an_unknown_codec():
    lib = pkg.lib()
    d = ctypes.c_void_p(16)
    for codec in (BC7, 99):
        assert lib.icamd_encode_etc2_device(codec, 2, 1, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, None) == -4
        assert lib.icamd_encode_etc2_colour_device(codec, 2, 1, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, None) == -4
        assert lib.icamd_encode_mips_device(codec, 2, 4, 0, 8, 8, 32, 1, 1, 0, 0, d, d, None, 0, None) == -4
        assert lib.icamd_encode_etc2_mips_device(codec, 2, 0, 4, 0, 0, 8, 8, 32, 1, 1, 0, 0, d, d, None, 0, None) == -4
        assert lib.icamd_encode_eac11_16_device(codec, 2, 8, 8, 8, 8, 32, 0, 0, 0, d, d, None) == -4
        assert lib.icamd_decode_eac11_16_device(codec, 8, 8, 0, 0, 0, 0, d, d, None) == -4
        assert lib.icamd_measure_error_eac11_16_device(codec, 2, 8, 8, 8, 8, 32, 0, 0, 0, d, d, d, None) == -4
        assert pkg.mip_chain_size(codec, 64, 64, 3) == (0, None)
        assert lib.icamd_mip_workspace_size(codec, 4, 64, 64, 3, 1) == 0
        for comps in (3, 4):
            assert pkg.mip_kernel_name(codec, comps) == "" and pkg.etc2_mip_kernel_name(codec, comps) == ""
            assert pkg.eac11_16_kernel_name(codec, comps) == "" and pkg.eac11_16_kernel_name(codec, comps, metric=True) == ""
            for modes in (0, 1, 2):  # (mode 0 names what the call forwards to for the codecs it takes: not this one)
                assert pkg.etc2_colour_kernel_name(codec, comps, modes) == "" and pkg.etc2_kernel_name(codec, comps, modes) == ""
    # no Compressor + format pair selects it: the size queries know three compressors only
    assert all(lib.icamd_supports_format(c, f) in (0, 1) for c in range(3) for f in range(4))


def test_prototype_table_still_matches_the_header():
    import test_abi_exports as X
    assert X.prototype_mismatches(X.header_prototypes(), pkg.abi.PROTOTYPES) == []


def _levels(h, w, n):
    g = np.random.default_rng(3200 + n)
    return [g.integers(0, 256, B.encoded_size(max(1, h >> l), max(1, w >> l)), dtype=np.uint8).tobytes() for l in range(n)]


def _dds(h, w, levels):
    n = len(levels)
    return b"DDS " + struct.pack("<7I", 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000 | (0x20000 if n > 1 else 0), h, w, len(levels[0]), 0, n) + \
        bytes(44) + struct.pack("<2I4s5I", 32, 0x4, b"DX10", 0, 0, 0, 0, 0) + \
        struct.pack("<5I", 0x1000 | (0x8 | 0x400000 if n > 1 else 0), 0, 0, 0, 0) + struct.pack("<5I", 98, 3, 0, 1, 0) + b"".join(levels)


def _ktx(h, w, levels):
    return bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A]) + \
        struct.pack("<13I", 0x04030201, 0, 1, 0, 0x8E8C, 0x1908, w, h, 0, 0, 1, len(levels), 0) + \
        b"".join(struct.pack("<I", len(b)) + b for b in levels)


def _pvr(h, w, levels):
    return struct.pack("<IIQIIIIIIIII", 0x03525650, 0, 15, 0, 0, h, w, 1, 1, 1, len(levels), 0) + b"".join(levels)


@pytest.mark.parametrize("h,w,n", [(64, 64, 1), (64, 64, 7), (61, 59, 3), (5, 3, 1)])
def test_container_bytes(h, w, n):
    levels = _levels(h, w, n)
    for container, want in ((pkg.CONTAINER_DDS, _dds(h, w, levels)), (pkg.CONTAINER_KTX, _ktx(h, w, levels)),
                            (pkg.CONTAINER_PVR, _pvr(h, w, levels))):
        assert pkg.container_size(container, BC7, h, w, n) == len(want), container
        assert pkg.container_write(container, BC7, h, w, levels) == want, (container, h, w, n)
    assert pkg.container_size(pkg.CONTAINER_PKM, BC7, h, w, 1) == 0
    # the legacy DDS header of the other codecs is unchanged: 128 bytes, their FOURCC, nothing after it but the levels
    l5 = [bytes(pkg.encoded_size(pkg.DXT5, max(1, h >> l), max(1, w >> l))) for l in range(n)]
    dxt5 = pkg.container_write(pkg.CONTAINER_DDS, pkg.DXT5, h, w, l5)
    assert len(dxt5) == 128 + sum(map(len, l5)) and dxt5[84:88] == b"DXT5" and dxt5[:84] == _dds(h, w, l5)[:84].replace(
        struct.pack("<I", len(levels[0])), struct.pack("<I", len(l5[0])))


def test_pillow_reads_the_dx10_dds_the_library_writes():
    pytest.importorskip("PIL")
    from PIL import Image
    img = B.content("smooth", 20, 28, 4)
    blocks = B.oracle_encode(img)
    data = pkg.container_write(pkg.CONTAINER_DDS, BC7, 20, 28, [blocks])
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (28, 20)
    assert (np.asarray(im.convert("RGBA")).reshape(20, 28 * 4) == B.decode(blocks, 20, 28)).all()


# ---- build check: the new kernels keep everything in registers

def test_bc7_kernels_use_no_scratch(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    metas = {}
    for unit in ("bc7_kernels", "metric_kernels"):
        out = os.path.join(str(tmp_path), unit + ".s")
        subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(T.ROOT, "include"),
                               "-I" + CSRC, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, unit + ".hip")],
                              stderr=subprocess.DEVNULL)
        for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", open(out).read(), re.S):
            blk = m.group(0)
            metas[re.search(r"\.name:\s+(\S+)", blk).group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
    names = ["icamd_bc7_rgba8_kernel", "icamd_bc7_rgb888_kernel", "icamd_bc7_rgba8_narrow_kernel", "icamd_bc7_rgb888_narrow_kernel",
             "icamd_bc7_decode_kernel", "icamd_metric_bc7_rgb888_kernel", "icamd_metric_bc7_rgba8_kernel"]
    for n in names:
        assert n in metas, n
        assert metas[n] == 0, "%s uses %d bytes of scratch" % (n, metas[n])
