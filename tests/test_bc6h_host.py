"""CPU tier for BC6H (include/ic_amd.h ICAMD_BC6H_UF16 / ICAMD_BC6H_SF16).

* The decoder: the numpy restatement (tests/bc6h_oracle.py) and the host twin of csrc/bc6h_block.h (tests/host_emul/bc6h_emul.cc,
  -DICAMD_HOST_EMULATION) against the two committed fixtures (tests/golden/bc6h_decode_kat.bin, bc6h_bits_kat.bin: what an
  independent decoder makes of the blocks, every header and index bit of every mode pinned by a pair that differs in that bit
  alone), and the twin against the restatement in half bits on 4096 further blocks per format.
* The one-subset encoder: the twin byte for byte against the definition's restatement on every shape, layout and content, the
  closed form of step 2 against the definition for every T, the anchor exchange, the refit, the worked example.
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

import bc6h_oracle as B
import ic_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
KAT = os.path.join(HERE, "golden", "bc6h_decode_kat.bin")
BITS = os.path.join(HERE, "golden", "bc6h_bits_kat.bin")
pkg = importlib.import_module("image-compression_amd")
UF16, SF16 = B.BC6H_UF16, B.BC6H_SF16
CODECS = (UF16, SF16)
SHAPES = [(1, 1), (4, 4), (5, 3), (9, 2), (61, 59)]
PAD = 6  # bytes of row padding
PADDED = [(5, 3, 16, 16), (30, 30, 40, 48)]
U64P = ctypes.POINTER(ctypes.c_uint64)
i32 = ctypes.c_int32


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bc6h") / "libbc6h_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC,
                           "-I" + os.path.join(T.ROOT, "include"), "-o", so, os.path.join(EMUL_DIR, "bc6h_emul.cc")])
    L = ctypes.CDLL(so)
    L.bc6h_emul_encode.restype = ctypes.c_int
    L.bc6h_emul_encode.argtypes = [T.ci, T.ci, T.u32, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp]
    L.bc6h_emul_decode.restype = ctypes.c_int
    L.bc6h_emul_decode.argtypes = [T.ci, T.u32, T.u32, T.u32, T.vp, T.vp]
    L.bc6h_emul_metric.restype = ctypes.c_int
    L.bc6h_emul_metric.argtypes = [T.ci, T.ci, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp, U64P]
    L.bc6h_emul_quantise.restype = i32
    L.bc6h_emul_quantise.argtypes = [T.ci, i32]
    L.bc6h_emul_endpoint_value.restype = i32
    L.bc6h_emul_endpoint_value.argtypes = [T.ci, i32]
    yield L
    T.assert_no_emul_violations(L, "test_bc6h_host")


def emul_encode(L, img, signed, gh=None, gw=None, pad=0):
    h, w, chans = img.shape
    out = np.zeros(B.encoded_size(max(h, gh or h), max(w, gw or w)), np.uint8)
    rows = np.zeros((h, w * chans + pad // 2), np.uint16)
    rows[:, :w * chans] = img.reshape(h, w * chans)
    assert L.bc6h_emul_encode(int(signed), chans, h, w, gh or h, gw or w, w * chans * 2 + pad, rows.ctypes.data, out.ctypes.data)
    return out.tobytes()


def emul_decode(L, blocks, h, w, signed, pad=0):
    out = np.zeros((h, w * 4 + pad // 2), np.uint16)
    b = np.frombuffer(bytes(blocks), np.uint8).copy()
    assert L.bc6h_emul_decode(int(signed), h, w, pad, b.ctypes.data, out.ctypes.data)
    return out


def emul_texels(L, blocks, signed):
    """n blocks -> [n, 16, 3] uint16 half bits through the twin (the blocks as a 4-row image)."""
    n = len(bytes(blocks)) // 16
    rows = emul_decode(L, blocks, 4, 4 * n, signed).reshape(4, n, 4, 4)
    assert (rows[..., 3] == 0x3C00).all()
    return rows.transpose(1, 0, 2, 3).reshape(n, 16, 4)[..., :3]


@functools.lru_cache(maxsize=None)
def kat():
    rec = np.fromfile(KAT, np.uint8).reshape(-1, 65)
    assert rec.shape[0] == 804
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def bits_kat():
    raw = open(BITS, "rb").read()
    n_partners, n_cells = struct.unpack_from("<2I", raw)
    partners = np.frombuffer(raw, np.uint8, n_partners * 65, 8).reshape(n_partners, 65)
    cells = np.frombuffer(raw, np.uint8, n_cells * 27, 8 + n_partners * 65).reshape(n_cells, 27)
    assert 8 + n_partners * 65 + n_cells * 27 == len(raw)
    return partners, cells


# ---- decoder

def test_fixtures_hold_every_cell_the_generator_promises():
    rec = kat()
    for signed in (0, 1):
        r = rec[rec[:, 16] == signed]
        assert len(r) == 402
        modes = [B.mode_of(int(b)) for b in r[:, 0]]
        assert [modes.count(m) for m in range(14)] == [33] * 10 + [17] * 4 and modes.count(-1) == 4
        for m in range(10):
            parts = sorted((int.from_bytes(bytes(b), "little") >> 77) & 31 for b, mm in zip(r[:320, :16], modes) if mm == m)
            assert parts == list(range(32)), m
        assert not r[-4:, 17:].any()  # reserved mode fields: zeros
        inner = ((r[:, 17:] > 0) & (r[:, 17:] < 255)).mean()
        assert inner >= (1 / 8 if signed else 1 / 5), inner
    # the bit sweep: every (format, mode, bit above the mode field) exactly once, block = partner with that one bit flipped
    partners, cells = bits_kat()
    seen = set()
    for c in cells:
        pi = int(c[17]) | int(c[18]) << 8
        p = partners[pi]
        x = int.from_bytes(bytes(c[:16]), "little") ^ int.from_bytes(bytes(p[:16]), "little")
        assert x and x & (x - 1) == 0 and c[16] == p[16]
        mode = B.mode_of(int(c[0]))
        assert mode == B.mode_of(int(p[0])) and mode >= 0
        assert bytes(c[19:]) != B.digest(p[17:])  # the pair differs visibly
        seen.add((int(c[16]), mode, x.bit_length() - 1))
    want = {(s, m, bit) for s in (0, 1) for m in range(14) for bit in range(B.MODES[m][1], 128)}
    assert seen == want and len(cells) == len(want) == 3456


def _check_fixtures(decode_texels):
    """decode_texels(blocks bytes, signed) -> [n, 16, 3] half bits; held to both fixtures."""
    partners, cells = bits_kat()
    for signed in (0, 1):
        for rec in (kat(), partners):
            r = rec[rec[:, 16] == signed]
            got = B.half_to_byte(decode_texels(r[:, :16].tobytes(), bool(signed))).reshape(-1, 48)
            bad = np.flatnonzero((got != r[:, 17:]).any(axis=1))
            assert len(bad) == 0, (signed, bad[:8])
        c = cells[cells[:, 16] == signed]
        got = B.half_to_byte(decode_texels(c[:, :16].tobytes(), bool(signed))).reshape(-1, 48)
        bad = [i for i in range(len(c)) if B.digest(got[i]) != bytes(c[i, 19:])]
        assert not bad, (signed, bad[:8])


def test_oracle_decodes_both_fixtures():
    _check_fixtures(B.decode_blocks)


def test_twin_decodes_both_fixtures(emul):
    _check_fixtures(lambda blocks, signed: emul_texels(emul, blocks, signed))


@pytest.mark.parametrize("signed", [False, True])
def test_twin_matches_oracle_in_half_bits_on_4096_stratified_blocks(emul, signed):
    blocks = B.stratified_blocks(4096, 0xB6 + int(signed))
    want = B.decode_blocks(blocks, signed)
    got = emul_texels(emul, blocks, signed)
    assert (got == want).all()
    modes = [B.mode_of(b) for b in blocks[::16]]
    assert all(modes.count(m) >= 227 for m in range(-1, 14))


def test_decoder_known_answers(emul):
    for e, half in ((100, 3115), (300, 9315), (400, 12415), (480, 14895), (495, 15360), (1023, 31743)):
        v = 0b00011
        for pos in (5, 15, 25, 35, 45, 55):
            v |= e << pos
        block = v.to_bytes(16, "little")
        assert (B.decode_blocks(block, False) == half).all() and (emul_texels(emul, block, False) == half).all()
    assert list(B.half_to_byte(np.array([3115, 9315, 12415, 14895, 15360], np.uint16))) == [0, 4, 35, 197, 255]


@pytest.mark.parametrize("signed", [False, True])
def test_decoder_padded_rows_and_clipped_shapes(emul, signed):
    for h, w in SHAPES:
        blocks = B.stratified_blocks(B.encoded_size(h, w) // 16, 31 * h + w)
        for pad in (0, PAD):
            want = B.decode(blocks, h, w, signed, pad)
            assert (emul_decode(emul, blocks, h, w, signed, pad) == want).all(), (h, w, pad)


# ---- encoder

def _images(h, w, chans):
    return [(name, B.content(name, h, w, chans)) for name in B.CONTENTS]


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("chans", [3, 4])
def test_encoder_matches_definition_on_every_shape_and_content(emul, signed, chans):
    for h, w in SHAPES:
        for name, img in _images(h, w, chans):
            want = B.oracle_encode(img, signed)
            assert emul_encode(emul, img, signed) == want, (name, h, w)
            assert emul_encode(emul, img, signed, pad=PAD) == want, (name, h, w, "padded rows")


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("h,w,gh,gw", PADDED)
def test_encoder_padded_grid(emul, signed, h, w, gh, gw):
    for chans in (3, 4):
        for name, img in _images(h, w, chans):
            want = B.oracle_encode(img, signed, gh, gw)
            assert len(want) == B.encoded_size(gh, gw)
            assert emul_encode(emul, img, signed, gh, gw) == want, (name, chans)


def test_contents_hold_what_they_promise():
    spec = B.content("specials", 61, 59, 4)
    for v in (0x7E00, 0x7C00, 0xFC00, 0x8000, 0x0001, 0x7BFF, 0xFBFF):
        assert (spec == v).any(), hex(v)
    exps = (B.content("exponents", 61, 59, 3).astype(np.int64) >> 10) & 31
    blocks = exps[:60, :56].reshape(15, 4, 14, 4, 3).transpose(0, 2, 1, 3, 4).reshape(-1, 48)
    assert (blocks.max(axis=1) - blocks.min(axis=1) >= 20).all()
    assert (B.content("noise", 61, 59, 3) & 0x8000).any()  # negatives reach the unsigned format
    flat = B.content("flat", 16, 16, 3)
    assert (flat[:8, :8] == flat[0, 0]).all()
    two = B.content("two_valued", 16, 16, 3)[:8, :8, 0]
    assert len(np.unique(two)) == 2


def test_target_map():
    h = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x3C00, 0xBC00, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7C01, 0xFE00], np.uint16)
    assert list(B.target(h, False)) == [0, 0, 1, 0, 15360, 0, 31743, 0, 31743, 0, 0, 0]
    assert list(B.target(h, True)) == [0, 0, 1, -1, 15360, -15360, 31743, -31743, 31743, -31743, 0, 0]
    # monotone in the float's value over every finite half
    allh = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    f = allh.view(np.float16).astype(np.float64)
    fin = np.isfinite(f)
    order = np.argsort(f[fin], kind="stable")
    for signed in (False, True):
        t = B.target(allh, signed)[fin][order]
        assert (np.diff(t) >= 0).all()


@pytest.mark.parametrize("signed", [False, True])
def test_step_2_closed_form_equals_the_definition_for_every_target(emul, signed):
    lo, hi = (-B.T_MAX, B.T_MAX) if signed else (0, B.T_MAX)
    T_all = np.arange(lo, hi + 1)
    want = B.quantise(T_all, signed)
    got = np.array([emul.bc6h_emul_quantise(int(signed), int(t)) for t in T_all])
    assert (got == want).all()
    qlo, qhi = B.q_range(signed)
    q = np.arange(qlo, qhi + 1)
    d = np.array([emul.bc6h_emul_endpoint_value(int(signed), int(x)) for x in q])
    assert (d == B.D(q, signed)).all() and (np.diff(d) > 0).all()
    assert d[-1] == 31743 and (d[0] == -31743 if signed else d[0] == 0)
    assert want.min() == qlo and want.max() == qhi  # (the signed encoder never writes -512)


@pytest.mark.parametrize("signed", [False, True])
def test_anchor_exchange_refit_and_invariants(signed):
    t = np.concatenate([B.block_texels(B.content(name, 32, 32, 3, seed=3), signed) for name in B.CONTENTS])
    blocks, sse, final, take, (e0, e1, k) = B.encode_texels(t, signed, stages=True)
    assert (final <= sse).all() and take.any() and (final[take] < sse[take]).all()  # no block's error exceeds its first pass's
    flip = k[:, 0] >= 8
    assert flip.any() and (~flip).any()
    # the decoded texels of the written block are the palette entries the search chose: the exchange changed nothing
    dec = B.decode_blocks(blocks.tobytes(), signed)
    pal = B.palette(e0, e1, signed)  # before the exchange
    chosen = np.take_along_axis(pal, k[:, :, None], axis=1)
    assert (B.target(dec, signed) == chosen).all()
    assert (((chosen - t) ** 2).sum(axis=(1, 2)) == final).all()
    assert (blocks[:, 0] & 31 == 3).all() and ((blocks[:, 8] >> 1) & 7 < 8).all()
    idx0 = (np.array([int.from_bytes(bytes(b), "little") >> 65 for b in blocks]) & 7)
    assert (idx0 == np.where(flip, 15 - k[:, 0], k[:, 0])).all()


def test_worked_example_blocks(emul):
    img = np.zeros((4, 4, 3), np.uint16)
    img[...] = (0x3C00, 0x3800, 0x3400)
    for signed, text in ((False, "e3 3d e7 5a 7b cf b9 d6"), (True, "e3 9e 73 ac b9 e7 1c 6b")):
        want = bytes.fromhex(text) + bytes(8)
        assert B.oracle_encode(img, signed) == want and emul_encode(emul, img, signed) == want


# ---- metric

@pytest.mark.parametrize("signed", [False, True])
def test_metric_twin_matches_numpy(emul, signed):
    for (h, w, gh, gw) in [(61, 59, 61, 59), (5, 3, 16, 16), (30, 30, 40, 48)]:
        for chans in (3, 4):
            img = B.content("noise" if chans == 3 else "gradient", h, w, chans)
            blocks = np.frombuffer(B.stratified_blocks(B.encoded_size(gh, gw) // 16, h + chans), np.uint8).copy()
            blocks[:160] = np.frombuffer(B.oracle_encode(img, signed, gh, gw), np.uint8)[:160]
            out = (ctypes.c_uint64 * 6)()
            src = np.ascontiguousarray(img)
            assert emul.bc6h_emul_metric(int(signed), chans, h, w, gw, w * chans * 2, src.ctypes.data, blocks.ctypes.data, out)
            sse, mx = B.metric(img, blocks.tobytes(), signed, gw)
            assert list(out)[:3] == list(sse) and list(out)[3:] == list(mx), (h, w, chans)


# ---- the C ABI's host-side surface (no device work: every check below returns before the GPU is touched)

def _name(codec, chans, metric=False):
    if codec not in CODECS or chans not in (3, 4):
        return ""
    return "icamd_%sbc6h_%s_%s_kernel" % ("metric_" if metric else "", "uf16" if codec == UF16 else "sf16", "rgb16f" if chans == 3 else "rgba16f")


def test_codec_values_sizes_and_kernel_names():
    assert (pkg.BC6H_UF16, pkg.BC6H_SF16) == (34, 35) == CODECS
    for codec in CODECS:
        assert pkg.encoded_size(codec, 8, 8) == 64 and pkg.encoded_size(codec, 5, 3) == 32
        assert pkg.encoded_size(codec, 257, 1023) == 65 * 256 * 16
    for codec in list(CODECS) + [0, 5, 25, 32, 33, 36]:
        for chans in range(0, 6):
            assert pkg.bc6h_kernel_name(codec, chans) == _name(codec, chans), (codec, chans)
            assert pkg.bc6h_kernel_name(codec, chans, metric=True) == _name(codec, chans, True), (codec, chans)
    assert pkg.psnr_bc6h_from_stats([0, 0, 0, 0], 16) == float("inf")
    assert abs(pkg.psnr_bc6h_from_stats([31743 ** 2 * 16, 0, 0, 0], 16, 1)) < 1e-9


def test_encode_statuses():
    lib = pkg.lib()
    enc = lib.icamd_encode_bc6h_device
    d = ctypes.c_void_p(16)  # never dereferenced: the arguments are refused first
    for codec in CODECS:
        for chans in range(0, 6):
            ok = chans in (3, 4)
            stride = 16 * max(chans, 1)
            for n in (0, 1) if not ok else (0,):
                assert enc(codec, chans, 8, 8, 8, 8, stride, n, 0, 0, d, d, None) == (0 if ok else -4), (codec, chans, n)
        c = 3
        assert enc(codec, c, 0, 8, 8, 8, 16 * c, 1, 0, 0, d, d, None) == 1       # empty image
        assert enc(codec, c, 8, 0, 8, 8, 16 * c, 1, 0, 0, d, d, None) == 1
        assert enc(codec, c, 8, 8, 8, 8, 16 * c, 1, 0, 0, None, d, None) == 1    # null source
        assert enc(codec, c, 8, 8, 8, 8, 16 * c, 1, 0, 0, d, None, None) == 1    # null output
        assert enc(codec, 9, 0, 8, 8, 8, 16 * c, 1, 0, 0, d, d, None) == 1       # ICAMD_FALSE comes first
        assert enc(codec, c, 8, 8, 8, 8, 16 * c, 0, 0, 0, d, d, None) == 0       # no images
        assert enc(codec, c, 8, 8, 8, 8, 16 * c - 2, 0, 0, 0, d, d, None) == 0   # no images: before the stride check
        assert enc(codec, c, 8, 8, 8, 8, 16 * c - 2, 1, 0, 0, d, d, None) == -4  # stride < row
        assert b"row stride" in lib.icamd_last_error()
        for n in (0, 1):  # 2-byte alignment is a rule: refused whatever the count
            assert enc(codec, c, 8, 8, 8, 8, 16 * c, n, 0, 0, ctypes.c_void_p(17), d, None) == -4
            assert b"even" in lib.icamd_last_error()
            assert enc(codec, c, 8, 8, 8, 8, 16 * c + 1, n, 0, 0, d, d, None) == -4
            assert enc(codec, c, 8, 8, 8, 8, 16 * c, n, 1001, 0, d, d, None) == -4
        assert enc(codec, c, 8, 8, 8, 8, 16 * c, 0, 0, 0, d, ctypes.c_void_p(17), None) == 0  # the output: any alignment
    for codec in (-1, 0, 5, 16, 24, 32, 33, 36):
        assert enc(codec, 3, 8, 8, 8, 8, 48, 0, 0, 0, d, d, None) == -4, codec


def test_decode_statuses():
    lib = pkg.lib()
    dec = lib.icamd_decode_bc6h_device
    d = ctypes.c_void_p(16)
    for codec in CODECS:
        assert dec(codec, 0, 8, 0, 1, 0, 0, d, d, None) == 1
        assert dec(codec, 8, 0, 0, 1, 0, 0, d, d, None) == 1
        assert dec(codec, 8, 8, 0, 1, 0, 0, None, d, None) == 1
        assert dec(codec, 8, 8, 0, 1, 0, 0, d, None, None) == 1
        assert dec(codec, 8, 8, 0, 0, 0, 0, d, d, None) == 0
        assert dec(codec, 8, 8, 6, 0, 0, 0, ctypes.c_void_p(17), d, None) == 0  # the blocks: any alignment
        for n in (0, 1):
            assert dec(codec, 8, 8, 3, n, 0, 0, d, d, None) == -4                 # odd padding
            assert dec(codec, 8, 8, 0, n, 0, 0, d, ctypes.c_void_p(17), None) == -4
            assert dec(codec, 8, 8, 0, n, 0, 1001, d, d, None) == -4
        assert dec(codec, 8, 0x20000000, 0, 0, 0, 0, d, d, None) == -4          # a row of 2^32 bytes or more
        assert dec(codec, 8, 0x1fffffff, 6, 0, 0, 0, d, d, None) == 0
    for codec in (-1, 0, 5, 16, 24, 32, 33, 36):
        assert dec(codec, 8, 8, 0, 0, 0, 0, d, d, None) == -4, codec
        assert dec(codec, 0, 8, 0, 0, 0, 0, d, d, None) == 1


def test_measure_statuses():
    lib = pkg.lib()
    met = lib.icamd_measure_error_bc6h_device
    d = ctypes.c_void_p(16)
    for codec in CODECS:
        for chans in range(0, 6):
            want = 0 if chans in (3, 4) else -4
            assert met(codec, chans, 8, 8, 8, 8, 16 * max(chans, 1), 0, 0, 0, d, d, d, None) == want, (codec, chans)
        c = 3
        assert met(codec, c, 0, 8, 8, 8, 16 * c, 1, 0, 0, d, d, d, None) == 1
        assert met(codec, c, 8, 8, 8, 8, 16 * c, 1, 0, 0, None, d, d, None) == 1
        assert met(codec, c, 8, 8, 8, 8, 16 * c, 1, 0, 0, d, None, d, None) == 1
        assert met(codec, c, 8, 8, 8, 8, 16 * c, 1, 0, 0, d, d, None, None) == 1
        assert met(codec, c, 8, 8, 8, 8, 16 * c, 0, 0, 0, d, d, d, None) == 0
        assert met(codec, c, 8, 8, 8, 8, 16 * c - 2, 0, 0, 0, d, d, d, None) == -4              # stride < row
        assert met(codec, c, 8, 8, 4, 8, 16 * c, 0, 0, 0, d, d, d, None) == -4                  # grid < image
        assert met(codec, c, 8, 8, 8, 4, 16 * c, 0, 0, 0, d, d, d, None) == -4
        assert met(codec, c, 8, 8, 8, 8, 16 * c, 0, 0, 0, d, d, ctypes.c_void_p(20), None) == -4  # d_stats alignment
        assert met(codec, c, 8, 8, 8, 8, 16 * c, 0, 0, 0, ctypes.c_void_p(17), d, d, None) == -4
        assert met(codec, c, 8, 8, 8, 8, 16 * c + 1, 0, 0, 0, d, d, d, None) == -4
        assert met(codec, c, 8, 8, 8, 8, 16 * c, 0, 1001, 0, d, d, d, None) == -4
        assert met(codec, c, 8, 8, 8, 8, 16 * c, 0, 0, 1001, d, ctypes.c_void_p(17), d, None) == 0  # the blocks: any alignment
        # (uint64) height * width > 2^31
        assert met(codec, c, 1 << 16, 1 << 15, 1 << 16, 1 << 15, (1 << 16) * c, 0, 0, 0, d, d, d, None) == 0
        assert met(codec, c, (1 << 16) + 1, 1 << 15, (1 << 16) + 1, 1 << 15, (1 << 16) * c, 0, 0, 0, d, d, d, None) == -4
    for codec in (-1, 0, 5, 16, 24, 32, 33, 36):
        assert met(codec, 3, 8, 8, 8, 8, 48, 0, 0, 0, d, d, d, None) == -4, codec


def test_33_is_still_unassigned_and_the_old_entry_points_refuse_bc6h():
    lib = pkg.lib()
    d = ctypes.c_void_p(16)
    for codec in (33, UF16, SF16):
        for comps in (1, 2, 3, 4):
            assert pkg.kernel_name(codec, comps) == "" and pkg.metric_kernel_name(codec, comps) == ""
            assert pkg.mip_kernel_name(codec, comps) == ""
            assert pkg.eac11_16_kernel_name(codec, comps) == "" and pkg.eac11_16_kernel_name(codec, comps, metric=True) == ""
            assert pkg.bc7_kernel_name(comps, pkg.BC7_MODES_EXTENDED) in ("", "icamd_bc7_modes_rgb888_kernel", "icamd_bc7_modes_rgba8_kernel")
        # the statuses an unknown codec gets, family by family
        for comps in (3, 4):
            assert lib.icamd_encode_device(codec, 2, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, None) == \
                lib.icamd_encode_device(99, 2, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, None)
            assert lib.icamd_measure_error_device(codec, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, d, None) == \
                lib.icamd_measure_error_device(99, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, d, None) == -4
        assert lib.icamd_decode_device(codec, 0, 8, 8, 0, 1, 0, 0, d, d, None) == lib.icamd_decode_device(99, 0, 8, 8, 0, 1, 0, 0, d, d, None) == 1
        assert lib.icamd_encode_etc2_device(codec, 2, 1, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, None) == -4
        assert lib.icamd_encode_etc2_colour_device(codec, 2, 1, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, None) == -4
        assert lib.icamd_encode_mips_device(codec, 2, 4, 0, 8, 8, 32, 1, 1, 0, 0, d, d, None, 0, None) == -4
        assert lib.icamd_encode_etc2_mips_device(codec, 2, 0, 4, 0, 0, 8, 8, 32, 1, 1, 0, 0, d, d, None, 0, None) == -4
        assert lib.icamd_encode_eac11_16_device(codec, 3, 8, 8, 8, 8, 48, 0, 0, 0, d, d, None) == -4
        assert lib.icamd_decode_eac11_16_device(codec, 8, 8, 0, 0, 0, 0, d, d, None) == -4
        assert lib.icamd_measure_error_eac11_16_device(codec, 3, 8, 8, 8, 8, 48, 0, 0, 0, d, d, d, None) == -4
        assert pkg.mip_chain_size(codec, 64, 64, 3) == (0, None)
        assert lib.icamd_mip_workspace_size(codec, 4, 64, 64, 3, 1) == 0
        assert pkg.etc2_mip_kernel_name(codec, 4) == ""
        for container in (pkg.CONTAINER_PKM, pkg.CONTAINER_PVR):
            assert pkg.container_size(container, codec, 8, 8, 1) == 0
    for container in (pkg.CONTAINER_DDS, pkg.CONTAINER_KTX):
        assert pkg.container_size(container, 33, 8, 8, 1) == 0
    assert pkg.bc6h_kernel_name(33, 3) == ""
    assert lib.icamd_container_write(pkg.CONTAINER_KTX, 33, 8, 8, 1, None, None, None, 0) == -4  # unknown codec


def test_prototype_table_still_matches_the_header():
    import test_abi_exports as X
    header = X.header_prototypes()
    new = ["icamd_encode_bc6h_device", "icamd_decode_bc6h_device", "icamd_measure_error_bc6h_device", "icamd_bc6h_kernel_name",
           "icamd_bc6h_metric_kernel_name"]
    assert all(n in header for n in new)
    assert X.prototype_mismatches(header, pkg.abi.PROTOTYPES) == []
    names = [n for n, _, _ in pkg.abi.PROTOTYPES]
    assert names[names.index("icamd_eac11_16_metric_kernel_name") + 1:][:5] == new  # header order
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, n) for n in new)


# ---- containers

def _levels(h, w, n):
    g = np.random.default_rng(600 + n)
    return [g.integers(0, 256, B.encoded_size(max(1, h >> l), max(1, w >> l)), dtype=np.uint8).tobytes() for l in range(n)]


def _ktx(codec, h, w, levels):
    return bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A]) + \
        struct.pack("<13I", 0x04030201, 0, 1, 0, 0x8E8F if codec == UF16 else 0x8E8E, 0x1907, w, h, 0, 0, 1, len(levels), 0) + \
        b"".join(struct.pack("<I", len(b)) + b for b in levels)


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("h,w,n", [(64, 64, 1), (64, 64, 7), (61, 59, 3), (5, 3, 1)])
def test_container_bytes(codec, h, w, n):
    levels = _levels(h, w, n)
    want = _ktx(codec, h, w, levels)
    assert pkg.container_size(pkg.CONTAINER_KTX, codec, h, w, n) == len(want)
    assert pkg.container_write(pkg.CONTAINER_KTX, codec, h, w, levels) == want
    dds = pkg.container_write(pkg.CONTAINER_DDS, codec, h, w, levels)
    assert len(dds) == pkg.container_size(pkg.CONTAINER_DDS, codec, h, w, n) == 148 + sum(len(b) for b in levels)
    # the BC7 file differs in dxgiFormat alone
    bc7 = pkg.container_write(pkg.CONTAINER_DDS, 32, h, w, levels)
    assert [i for i in range(len(dds)) if dds[i] != bc7[i]] == [128]
    assert dds[128] == (95 if codec == UF16 else 96) and dds[84:88] == b"DX10"
    for container in (pkg.CONTAINER_PKM, pkg.CONTAINER_PVR):  # refused as for a codec the container cannot hold
        assert pkg.container_size(container, codec, h, w, n) == 0
        assert pkg.container_write(container, codec, h, w, levels) is None


@pytest.mark.parametrize("signed", [False, True])
def test_dds_opens_in_pillow_and_gives_the_oracles_bytes(signed):
    Image = pytest.importorskip("PIL.Image")
    h, w = 20, 36
    codec = SF16 if signed else UF16
    img = B.content("ldr", h, w, 3)
    img[:8] = B.content("gradient", 8, w, 3)
    blocks = B.oracle_encode(img, signed)
    mixed = B.stratified_blocks(len(blocks) // 16, 77)
    for stream in (blocks, mixed):
        data = pkg.container_write(pkg.CONTAINER_DDS, codec, h, w, [stream])
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.size == (w, h) and im.mode == "RGB"
        want = B.half_to_byte(B.decode(stream, h, w, signed).reshape(h, w, 4)[..., :3])
        assert (np.asarray(im) == want).all()


# ---- build check: the new kernels keep everything in registers

def test_bc6h_kernels_use_no_scratch(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "bc6h_kernels.s")
    subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(T.ROOT, "include"),
                           "-I" + CSRC, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "bc6h_kernels.hip")],
                          stderr=subprocess.DEVNULL)
    metas = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", open(out).read(), re.S):
        blk = m.group(0)
        metas[re.search(r"\.name:\s+(\S+)", blk).group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
    names = [_name(c, n) for c in CODECS for n in (3, 4)]
    names += [n.replace("_kernel", "_narrow_kernel") for n in names] + [_name(c, n, True) for c in CODECS for n in (3, 4)]
    names += ["icamd_bc6h_uf16_decode_kernel", "icamd_bc6h_sf16_decode_kernel"]
    assert len(names) == 14
    for n in names:
        assert n in metas, n
        assert metas[n] == 0, "%s uses %d bytes of scratch" % (n, metas[n])
