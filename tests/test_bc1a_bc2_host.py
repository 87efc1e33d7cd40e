"""CPU tier for ICAMD_BC1A (BC1 with punch-through alpha) and ICAMD_BC2 (include/ic_amd.h).

* The numpy statement (tests/bc1a_bc2_oracle.py) against the committed fixture, whose expected bytes are Pillow's.
* The block math of image-compression_amd/csrc/bc1a_block.h compiled for the host (tests/host_emul/bc1a_bc2_emul.cc,
  -DICAMD_HOST_EMULATION), bit-exact against the numpy statement: both decoders, both encoders, padded grids, four masks, both
  swap_rb values; the worked examples of the header as literals.
* Exact properties of the encoders, the classes of block the inputs must hold, the constant-colour proof over all 2^24 colours.
* The C ABI's host-side surface of codecs 36 and 37: sizes, kernel names, the ICAMD_ERR_ARG cases, the other families' refusals,
  container headers field by field, a DDS through Pillow.
* The new kernels compile without scratch and without spills (code-object metadata only)."""
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

import bc1a_bc2_oracle as O
import ic_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
pkg = importlib.import_module("image-compression_amd")
BC1A, BC2 = O.BC1A, O.BC2
PADDED = [(30, 30, 40, 48), (5, 3, 16, 16), (1, 1, 9, 13), (64, 61, 64, 64), (17, 33, 24, 48)]
CASES = [(mask, h, w, gh, gw) for mask in O.MASKS for h, w, gh, gw in PADDED]


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bc1a_bc2") / "libbc1a_bc2_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC,
                           "-I" + os.path.join(T.ROOT, "include"), "-o", so, os.path.join(EMUL_DIR, "bc1a_bc2_emul.cc")])
    L = ctypes.CDLL(so)
    L.bc1a_bc2_emul_encode.restype = ctypes.c_int
    L.bc1a_bc2_emul_encode.argtypes = [T.ci, T.ci, T.u32, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp]
    L.bc1a_emul_encode_masked.restype = None
    L.bc1a_emul_encode_masked.argtypes = [T.u32, T.ci, T.vp, T.vp]
    L.bc1a_bc2_emul_decode.restype = None
    L.bc1a_bc2_emul_decode.argtypes = [T.ci, T.u32, T.ci, T.vp, T.vp]
    L.bc1a_emul_const_scan.restype = None
    L.bc1a_emul_const_scan.argtypes = [T.vp, T.vp]
    yield L
    T.assert_no_emul_violations(L, "test_bc1a_bc2_host")


def emul_decode(L, codec, blocks, swap=0):
    size = O.BLOCK_BYTES[codec]
    b = np.frombuffer(bytes(blocks), np.uint8).copy()
    out = np.zeros((b.size // size, 4, 4, 4), np.uint8)
    L.bc1a_bc2_emul_decode(int(codec == BC2), b.size // size, swap, b.ctypes.data, out.ctypes.data)
    return out


def emul_encode(L, codec, flat, h, w, swap=0, gh=None, gw=None, stride=None):
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    out = np.zeros(O.encoded_size(codec, gh, gw), np.uint8)
    src = np.ascontiguousarray(flat, dtype=np.uint8).reshape(-1)
    assert L.bc1a_bc2_emul_encode(int(codec == BC2), swap, h, w, gh, gw, w * 4 if stride is None else stride, src.ctypes.data,
                                  out.ctypes.data)
    return out.tobytes()


def emul_encode_masked(L, tex, swap=0):
    """[n, 16, 4] canonical texels -> [n, 8] through the masked path alone."""
    mem = tex[..., [2, 1, 0, 3]] if swap else tex
    src = np.ascontiguousarray(mem, np.uint8).reshape(-1)
    out = np.zeros((tex.shape[0], 8), np.uint8)
    L.bc1a_emul_encode_masked(tex.shape[0], swap, src.ctypes.data, out.ctypes.data)
    return out


@functools.lru_cache(maxsize=None)
def _image(mask, h, w):
    return O.masked_image("mixed", mask, h, w, index=h + w)


@functools.lru_cache(maxsize=None)
def _want(codec, mask, h, w, gh, gw, swap):
    return O.oracle_encode(codec, _image(mask, h, w), h, w, swap, gh=gh, gw=gw)


@functools.lru_cache(maxsize=None)
def _random_masked():
    return O.random_masked_blocks(20000, seed=3600)


# ---- the statement against Pillow (the committed fixture), and the device decoders' math against the statement

def test_fixture_holds_the_cases_and_the_statement_agrees_with_pillow():
    bc1, dec1, bc2, dec2 = O.load_golden()
    assert bc1.shape == (256, 8) and bc2.shape == (256, 16)
    c0, c1, idx = O.colour_words(bc1)
    assert (c0 == c1).sum() >= 64 and (c0 > c1).sum() >= 64 and (c0 < c1).sum() >= 64
    assert all(((idx == k) & (c0 < c1)[:, None]).any() for k in range(4))
    d0, d1, _ = O.colour_words(bc2[:, 8:])
    assert (d0 <= d1).sum() >= 64 and (d0 > d1).sum() >= 64
    assert (O.decode_bc1a_blocks(bc1).reshape(-1, 64) == dec1).all()
    assert (O.decode_bc2_blocks(bc2).reshape(-1, 64) == dec2).all()
    # the transparent index is in the fixture, and c0 == c1 blocks decode index 3 clear, unlike ICAMD_DXT1's decoder
    assert (dec1.reshape(-1, 16, 4)[(idx == 3) & (c0 <= c1)[:, None]] == 0).all()
    assert ((idx == 3) & (c0 == c1)[:, None]).any()
    # c0 <= c1 colour words of BC2 are NOT three-colour: index 3 is opaque-coloured there
    assert (dec2.reshape(-1, 16, 4)[..., 3] == np.stack([bc2[:, p >> 1] >> (4 * (p & 1)) & 15 for p in range(16)], 1) * 17).all()


def test_generator_reproduces_the_fixture():
    PIL = pytest.importorskip("PIL")  # noqa: F841
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_bc1a_bc2_golden as G
    bc1, dec1, bc2, dec2 = O.load_golden()
    assert (O.random_bc1_blocks(G.N_BC1, G.SEED) == bc1).all() and (O.random_bc2_blocks(G.N_BC2, G.SEED + 16) == bc2).all()
    assert (G.pillow_decode(b"DXT1", bc1.tobytes(), 8) == dec1).all() and (G.pillow_decode(b"DXT3", bc2.tobytes(), 16) == dec2).all()


def test_decoders_on_the_fixture(emul):
    bc1, dec1, bc2, dec2 = O.load_golden()
    for codec, blocks, dec in ((BC1A, bc1, dec1), (BC2, bc2, dec2)):
        want = dec.reshape(-1, 4, 4, 4)
        assert (emul_decode(emul, codec, blocks) == want).all()
        assert (emul_decode(emul, codec, blocks, swap=1) == want[..., [2, 1, 0, 3]]).all()


def test_decoders_on_random_blocks(emul):
    n = 1 << 14
    for codec, blocks in ((BC1A, O.random_bc1_blocks(n, 3700)), (BC2, O.random_bc2_blocks(n, 3701))):
        want = O.decode_blocks(codec, blocks)
        assert (emul_decode(emul, codec, blocks) == want).all()
        assert (emul_decode(emul, codec, blocks, swap=1) == want[..., [2, 1, 0, 3]]).all()


# ---- the worked examples of the header, as literals

def test_worked_examples(emul):
    a, b = O.example_images()
    for img, block, texels in ((a, "b864b864f0f0f0f0", {0: (99, 150, 198, 255), 1: (99, 150, 198, 255), 2: (0, 0, 0, 0), 3: (0, 0, 0, 0)}),
                               (b, "a40826c3545955d5", {0: (8, 20, 33, 255), 1: (198, 101, 49, 255), 5: (103, 60, 41, 255),
                                                        15: (0, 0, 0, 0)})):
        assert O.oracle_encode(BC1A, img, 4, 4).hex() == block
        assert emul_encode(emul, BC1A, img, 4, 4).hex() == block
        swapped = np.ascontiguousarray(img[..., [2, 1, 0, 3]])  # the same colours in a BGRA buffer
        assert emul_encode(emul, BC1A, swapped, 4, 4, swap=1).hex() == block == O.oracle_encode(BC1A, swapped, 4, 4, 1).hex()
        for dec in (O.decode_bc1a_blocks(bytes.fromhex(block)), emul_decode(emul, BC1A, bytes.fromhex(block))):
            for p, want in texels.items():
                assert tuple(int(v) for v in dec.reshape(16, 4)[p]) == want, (block, p)
    dec = emul_decode(emul, BC1A, bytes.fromhex("b864b864f0f0f0f0"))[0]  # example 1: the whole columns
    assert (dec[:, :2] == (99, 150, 198, 255)).all() and (dec[:, 2:] == 0).all()


def test_all_transparent_word(emul):
    img = O.example_images()[0].copy()
    img[..., 3] = 127
    for swap in (0, 1):
        assert emul_encode(emul, BC1A, img, 4, 4, swap) == bytes.fromhex("00000000ffffffff") == O.oracle_encode(BC1A, img, 4, 4, swap)
    assert (emul_decode(emul, BC1A, bytes.fromhex("00000000ffffffff")) == 0).all()


def test_bc2_nibbles_for_all_256_alphas(emul):
    img = np.zeros((16, 16, 4), np.uint8)
    img[..., :3] = (90, 140, 30)
    img[..., 3] = np.arange(256).reshape(16, 16)
    want = np.floor(15 * np.arange(256) / 255.0 + 0.5).astype(np.int64)
    assert (O.quantize8(np.arange(256), 15) == want).all()
    assert [int(want[a]) for a in (0, 127, 128, 200, 255)] == [0, 7, 8, 12, 15]
    got = np.frombuffer(emul_encode(emul, BC2, img, 16, 16), np.uint8).reshape(4, 4, 16)
    for br in range(4):
        for bc in range(4):
            a = got[br, bc, :8].astype(np.int64)
            nib = np.array([a[p >> 1] >> (4 * (p & 1)) & 15 for p in range(16)]).reshape(4, 4)
            assert (nib == want[img[4 * br:4 * br + 4, 4 * bc:4 * bc + 4, 3]]).all()


# ---- encoders against the statement

@pytest.mark.parametrize("mask,h,w,gh,gw", CASES)
def test_encoders_match_statement(emul, mask, h, w, gh, gw):
    img = _image(mask, h, w)
    for codec in (BC1A, BC2):
        for swap in (0, 1):
            assert emul_encode(emul, codec, img, h, w, swap, gh=gh, gw=gw) == _want(codec, mask, h, w, gh, gw, swap), (codec, swap)


def test_row_padding(emul):
    h, w, pad = 13, 22, 5
    img = O.masked_image("smooth", "blobs", h, w, index=3)
    flat = T.with_row_padding(img, pad)
    for codec in (BC1A, BC2):
        assert emul_encode(emul, codec, flat, h, w, stride=w * 4 + pad) == O.oracle_encode(codec, img, h, w)


def test_masked_path_on_random_blocks(emul):
    tex = _random_masked()
    want = O.encode_masked(tex)
    for swap in (0, 1):
        assert (emul_encode_masked(emul, tex, swap) == want).all()
    eq = (want[:, 0] == want[:, 2]) & (want[:, 1] == want[:, 3])
    assert eq.any() and (~eq).any()  # c0 == c1 happens in the masked path, and is not the rule


def test_inputs_hold_every_class():
    blob = O.blob_fixture()
    shares = O.class_shares(blob, 64, 64)
    assert min(shares) >= 0.05, shares
    seen = set()
    for mask, h, w, gh, gw in CASES:
        _, cls = O.oracle_encode(BC1A, _image(mask, h, w), h, w, 0, gh=gh, gw=gw, return_classes=True)
        seen |= set(cls.tolist())
        if mask == "one":
            # (edge replication spreads the texel: the 1 x 1 image's blocks are all-transparent)
            assert (cls != 2).sum() >= 1 and ((cls == 1).sum() >= 1 or h * w == 1) and (np.asarray(_image(mask, h, w))[..., 3] < 128).sum() == 1
        if mask == "none":
            assert (cls == 2).all()
    assert seen == {0, 1, 2}


# ---- exact properties

def _property_inputs():
    for mask, h, w, gh, gw in CASES:
        for swap in (0, 1):
            yield _image(mask, h, w), h, w, gh, gw, swap
    yield O.blob_fixture(), 64, 64, 64, 64, 0


def test_bc1a_properties(emul):
    for img, h, w, gh, gw, swap in _property_inputs():
        tex = O.block_texels(img, h, w, gh, gw, swap)
        opq = tex[:, :, 3] >= 128
        got = np.frombuffer(emul_encode(emul, BC1A, img, h, w, swap, gh=gh, gw=gw), np.uint8).reshape(-1, 8)
        dec = O.decode_bc1a_blocks(got).reshape(-1, 16, 4)
        assert (dec[:, :, 3] == np.where(opq, 255, 0)).all()           # no texel gains or loses transparency
        c0, c1, idx = O.colour_words(got)
        # Three-colour mode beside transparency, always.  Without it c0 > c1, EXCEPT where the DXT1 bytes are its constant-colour
        # path's (darkest and brightest texel quantise to one 565 colour): that path stores equal endpoints with index 0 or the
        # "1/2" pair as c0 < c1 with index 2, never index 3 -- the block stays fully opaque (the alpha check above saw it).
        full = opq.all(axis=1)
        assert (c0 <= c1)[~full].all()
        lum = 4 * tex[:, :, 0] + 8 * tex[:, :, 1] + tex[:, :, 2]
        rows = np.arange(tex.shape[0])
        const = O.quantize565(tex[rows, lum.argmin(axis=1), :3]) == O.quantize565(tex[rows, lum.argmax(axis=1), :3])
        assert ((c0 > c1) | const)[full].all() and (c0 > c1)[full & ~const].all()
        assert not (idx[full & (c0 <= c1)] == 3).any()
        stored, best = O.research_error(tex, got)
        # re-searching the indices never lowers the error of a block of the masked path (the fully opaque blocks are the DXT1
        # bytes, whose indices are nearest in LUMINANCE by the reference's rule: an RGB re-search can beat those, by definition)
        assert (stored == best)[~full].all()
        forced = np.asarray(img).reshape(h, w, 4).copy()
        forced[..., 3] = 255
        assert emul_encode(emul, BC1A, forced, h, w, swap, gh=gh, gw=gw) == T.oracle_encode(T.DXT1, forced, h, w, 4, swap, gh=gh, gw=gw)
        dxt5 = np.frombuffer(T.oracle_encode(T.DXT5, img, h, w, 4, swap, gh=gh, gw=gw), np.uint8).reshape(-1, 16)
        bc2 = np.frombuffer(emul_encode(emul, BC2, img, h, w, swap, gh=gh, gw=gw), np.uint8).reshape(-1, 16)
        assert (bc2[:, 8:] == dxt5[:, 8:]).all()                        # BC2's colour half is DXT5's
        assert (O.decode_bc2_blocks(bc2).reshape(-1, 16, 4)[:, :, 3] == O.quantize8(tex[:, :, 3], 15) * 17).all()


def test_bc1a_properties_on_random_blocks(emul):
    tex = _random_masked()
    got = emul_encode_masked(emul, tex)
    dec = O.decode_bc1a_blocks(got).reshape(-1, 16, 4)
    assert (dec[:, :, 3] == np.where(tex[:, :, 3] >= 128, 255, 0)).all()
    c0, c1, _ = O.colour_words(got)
    assert (c0 <= c1).all()
    stored, best = O.research_error(tex, got)
    assert (stored == best).all()


def test_constant_colour_path_never_decodes_differently_under_bc1a(emul):
    """All 2^24 colours through the DXT1 colour block: whatever pair of the constant table it stores, the BC1A decoder reads
    sixteen opaque texels of the DXT1 decoder's colour, and equal endpoints come with index 0 only."""
    counts = (ctypes.c_uint64 * 4)()
    bad = (ctypes.c_uint64 * 2)()
    emul.bc1a_emul_const_scan(counts, bad)
    assert sum(counts) == 1 << 24 and list(bad) == [0, 0], (list(counts), list(bad))
    assert counts[0] > 0 and counts[2] > 0  # the plain colour and a blended pair both occur


# ---- the C ABI's host-side surface (no device work: every check below returns before the GPU is touched)

def test_codec_values_sizes_and_kernel_names():
    assert (pkg.BC1A, pkg.BC2) == (36, 37) == (BC1A, BC2)
    assert pkg.encoded_size(36, 8, 8) == 32 and pkg.encoded_size(37, 8, 8) == 64
    assert pkg.encoded_size(36, 5, 3) == 16 and pkg.encoded_size(37, 5, 3) == 32
    assert pkg.encoded_size(36, 257, 1023) == 65 * 256 * 8 and pkg.encoded_size(37, 257, 1023) == 65 * 256 * 16
    assert pkg.kernel_name(36, 4) == "icamd_bc1a_rgba8_kernel" and pkg.kernel_name(37, 4) == "icamd_bc2_rgba8_kernel"
    assert pkg.metric_kernel_name(36, 4) == "icamd_metric_bc1a_rgba8_kernel"
    assert pkg.metric_kernel_name(37, 4) == "icamd_metric_bc2_rgba8_kernel"
    for codec in (36, 37):
        for comps in (0, 1, 2, 3, 5):
            assert pkg.kernel_name(codec, comps) == "" and pkg.metric_kernel_name(codec, comps) == ""
    assert pkg.kernel_name(pkg.DXT1, 4) == "icamd_dxt1_rgba8_kernel" and pkg.kernel_name(pkg.DXT5, 4) == "icamd_dxt5_rgba8_kernel"
    header = open(os.path.join(T.ROOT, "include", "ic_amd.h")).read()
    assert "ICAMD_BC1A = 36, ICAMD_BC2 = 37" in header and "38 and up are unassigned" in header


def test_argument_errors():
    lib = pkg.lib()
    d = ctypes.c_void_p(16)  # never dereferenced: the arguments are refused first
    for codec in (36, 37):
        for comps in (0, 1, 2, 3, 5):
            assert lib.icamd_encode_device(codec, 2, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, None) == -4, (codec, comps)
            assert lib.icamd_last_error().decode() ==("BC1A" if codec == 36 else "BC2") + " needs a 4-component source"
            assert lib.icamd_measure_error_device(codec, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, d, None) == -4, (codec, comps)
        assert lib.icamd_encode_device(codec, 2, 4, 0, 0, 8, 8, 8, 32, 1, 0, 0, d, d, None) == 1    # empty image
        assert lib.icamd_encode_device(codec, 2, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, None, d, None) == 1  # null source
        assert lib.icamd_encode_device(codec, 2, 4, 0, 8, 8, 8, 8, 32, 0, 0, 0, d, d, None) == 0     # no images
        assert lib.icamd_decode_device(codec, 0, 8, 0, 0, 1, 0, 0, d, d, None) == 1
        assert lib.icamd_decode_device(codec, 0, 8, 8, 0, 1, 0, 0, None, d, None) == 1
        assert lib.icamd_decode_device(codec, 0, 8, 8, 0, 0, 0, 0, d, d, None) == 0
        assert lib.icamd_measure_error_device(codec, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, None, d, None) == 1
        assert lib.icamd_measure_error_device(codec, 4, 0, 8, 8, 8, 8, 31, 1, 0, 0, d, d, d, None) == -4  # stride < row
        assert lib.icamd_measure_error_device(codec, 4, 0, 8, 8, 4, 8, 32, 1, 0, 0, d, d, d, None) == -4  # grid < image
        assert lib.icamd_measure_error_device(codec, 4, 0, 8, 8, 8, 8, 32, 0, 0, 0, d, d, d, None) == 0   # no images


def test_every_other_family_refuses_them_as_codec_99_and_38_is_unassigned():
    lib = pkg.lib()
    d = ctypes.c_void_p(16)
    calls = [
        lambda c: lib.icamd_encode_etc2_device(c, 2, 1, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, None),
        lambda c: lib.icamd_encode_etc2_device(c, 2, 0, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, None),
        lambda c: lib.icamd_encode_etc2_colour_device(c, 2, 1, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, None),
        lambda c: lib.icamd_encode_etc2_colour_device(c, 2, 0, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, None),
        lambda c: lib.icamd_encode_mips_device(c, 2, 4, 0, 8, 8, 32, 1, 1, 0, 0, d, d, None, 0, None),
        lambda c: lib.icamd_encode_mips_filtered_device(c, 2, 4, 0, 0, 8, 8, 32, 1, 1, 0, 0, d, d, None, 0, None),
        lambda c: lib.icamd_encode_etc2_mips_device(c, 2, 0, 4, 0, 0, 8, 8, 32, 1, 1, 0, 0, d, d, None, 0, None),
        lambda c: lib.icamd_encode_eac11_16_device(c, 3, 8, 8, 8, 8, 48, 0, 0, 0, d, d, None),
        lambda c: lib.icamd_decode_eac11_16_device(c, 8, 8, 0, 0, 0, 0, d, d, None),
        lambda c: lib.icamd_measure_error_eac11_16_device(c, 3, 8, 8, 8, 8, 48, 0, 0, 0, d, d, d, None),
        lambda c: lib.icamd_encode_bc6h_device(c, 4, 8, 8, 8, 8, 64, 0, 0, 0, d, d, None),
        lambda c: lib.icamd_decode_bc6h_device(c, 8, 8, 0, 0, 0, 0, d, d, None),
        lambda c: lib.icamd_measure_error_bc6h_device(c, 4, 8, 8, 8, 8, 64, 0, 0, 0, d, d, d, None),
        lambda c: lib.icamd_mip_workspace_size(c, 4, 64, 64, 3, 1),
        lambda c: pkg.mip_chain_size(c, 64, 64, 3),
        lambda c: pkg.mip_kernel_name(c, 4),
        lambda c: pkg.etc2_mip_kernel_name(c, 4),
        lambda c: pkg.eac11_16_kernel_name(c, 4),
        lambda c: pkg.eac11_16_kernel_name(c, 4, metric=True),
        lambda c: lib.icamd_etc2_kernel_name(c, 4, 0),
        lambda c: lib.icamd_etc2_kernel_name(c, 4, 1),
        lambda c: lib.icamd_etc2_colour_kernel_name(c, 4, 0),
        lambda c: lib.icamd_etc2_colour_kernel_name(c, 4, 2),
        lambda c: lib.icamd_bc6h_kernel_name(c, 4),
        lambda c: lib.icamd_bc6h_metric_kernel_name(c, 4),
        lambda c: lib.icamd_bptc_mip_kernel_name(c, 4, 0),
        lambda c: pkg.container_size(pkg.CONTAINER_PKM, c, 8, 8, 1),
    ]
    for i, call in enumerate(calls):
        want = call(99)
        for codec in (36, 37, 38):
            assert call(codec) == want, (i, codec, want)
    assert pkg.mip_chain_size(36, 64, 64, 3) == (0, None) == pkg.mip_chain_size(37, 64, 64, 3)
    # 38 is unknown to the entry points that take 36 and 37
    for comps in (3, 4):
        assert pkg.kernel_name(38, comps) == "" and pkg.metric_kernel_name(38, comps) == ""
        assert lib.icamd_encode_device(38, 2, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, None) == \
            lib.icamd_encode_device(99, 2, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, None)
        assert lib.icamd_measure_error_device(38, comps, 0, 8, 8, 8, 8, 32, 1, 0, 0, d, d, d, None) == -4
    assert lib.icamd_decode_device(38, 0, 8, 8, 0, 1, 0, 0, d, d, None) == 1
    for container in (pkg.CONTAINER_DDS, pkg.CONTAINER_KTX, pkg.CONTAINER_PKM, pkg.CONTAINER_PVR):
        assert pkg.container_size(container, 38, 8, 8, 1) == 0
    # no Compressor + format pair selects them: the host-buffer families size DXT1 / DXT5 as before
    assert pkg.compute_compressed_data_size(pkg.COMPRESSOR_DXTC, pkg.RGBA, 8, 8) == 64
    assert pkg.compute_compressed_data_size(pkg.COMPRESSOR_DXTC, pkg.RGB, 8, 8) == 32


# ---- containers

def _levels(codec, h, w, n):
    g = np.random.default_rng(360 + n)
    return [g.integers(0, 256, ((max(1, h >> l) + 3) // 4) * ((max(1, w >> l) + 3) // 4) * O.BLOCK_BYTES[codec], dtype=np.uint8).tobytes()
            for l in range(n)]


def _dds(codec, h, w, levels):
    n = len(levels)
    flags = 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000 | (0x20000 if n > 1 else 0)
    caps = 0x1000 | (0x8 | 0x400000 if n > 1 else 0)
    pf_flags, fourcc = (0x5, b"DXT1") if codec == BC1A else (0x4, b"DXT3")
    return b"DDS " + struct.pack("<7I", 124, flags, h, w, len(levels[0]), 0, n) + bytes(44) + \
        struct.pack("<2I4s5I", 32, pf_flags, fourcc, 0, 0, 0, 0, 0) + struct.pack("<5I", caps, 0, 0, 0, 0) + b"".join(levels)


def _ktx(codec, h, w, levels):
    return bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A]) + \
        struct.pack("<13I", 0x04030201, 0, 1, 0, 0x83F1 if codec == BC1A else 0x83F2, 0x1908, w, h, 0, 0, 1, len(levels), 0) + \
        b"".join(struct.pack("<I", len(b)) + b for b in levels)


def _pvr(codec, h, w, levels):
    return struct.pack("<IIQIIIIIIIII", 0x03525650, 0, 7 if codec == BC1A else 9, 0, 0, h, w, 1, 1, 1, len(levels), 0) + b"".join(levels)


@pytest.mark.parametrize("h,w,n", [(64, 64, 1), (64, 64, 7), (61, 59, 3), (5, 3, 1)])
def test_container_bytes(h, w, n):
    for codec in (BC1A, BC2):
        levels = _levels(codec, h, w, n)
        for container, want in ((pkg.CONTAINER_DDS, _dds(codec, h, w, levels)), (pkg.CONTAINER_KTX, _ktx(codec, h, w, levels)),
                                (pkg.CONTAINER_PVR, _pvr(codec, h, w, levels))):
            assert pkg.container_size(container, codec, h, w, n) == len(want)
            assert pkg.container_write(container, codec, h, w, levels) == want, (codec, container, h, w, n)
        assert pkg.container_size(pkg.CONTAINER_PKM, codec, h, w, 1) == 0
        assert pkg.lib().icamd_container_write(pkg.CONTAINER_PKM, codec, h, w, 1, None, None, None, 0) == 1
    # the one difference between BC1A's DDS header and ICAMD_DXT1's is the DDPF_ALPHAPIXELS flag
    levels = _levels(BC1A, h, w, n)
    a = pkg.container_write(pkg.CONTAINER_DDS, BC1A, h, w, levels)
    b = pkg.container_write(pkg.CONTAINER_DDS, pkg.DXT1, h, w, levels)
    assert [i for i in range(len(a)) if a[i] != b[i]] == [80] and a[80] == 5 and b[80] == 4
    assert a[84:88] == b"DXT1" and pkg.container_write(pkg.CONTAINER_DDS, BC2, h, w, _levels(BC2, h, w, n))[84:88] == b"DXT3"


@pytest.mark.parametrize("codec", [BC1A, BC2])
def test_dds_opens_in_pillow(codec):
    Image = pytest.importorskip("PIL.Image")
    img = O.blob_fixture()
    blocks = O.oracle_encode(codec, img, 64, 64)
    im = Image.open(io.BytesIO(pkg.container_write(pkg.CONTAINER_DDS, codec, 64, 64, [blocks])))
    im.load()
    assert im.mode == "RGBA" and im.size == (64, 64)
    assert np.asarray(im).tobytes() == O.oracle_decode(codec, blocks, 64, 64).tobytes()


# ---- build check: the new kernels keep everything in registers (code-object metadata only)

def test_new_kernels_use_no_scratch_and_no_spills(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    metas = {}
    for unit in ("bc1a_bc2_kernels.hip", "decode_kernels.hip", "metric_kernels.hip"):
        out = os.path.join(str(tmp_path), unit + ".s")
        subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(T.ROOT, "include"),
                               "-I" + CSRC, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, unit)],
                              stderr=subprocess.DEVNULL)
        for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", open(out).read(), re.S):
            blk = m.group(0)
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            metas[name] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                           int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)))
    names = ["icamd_bc1a_rgba8_kernel", "icamd_bc1a_rgba8_narrow_kernel", "icamd_bc2_rgba8_kernel", "icamd_bc2_rgba8_narrow_kernel",
             "icamd_bc1a_decode_kernel", "icamd_bc2_decode_kernel", "icamd_metric_bc1a_rgba8_kernel", "icamd_metric_bc2_rgba8_kernel"]
    for n in names:
        assert n in metas, n
        assert metas[n] == (0, 0), "%s: %d bytes of scratch, %d spills" % ((n,) + metas[n])
