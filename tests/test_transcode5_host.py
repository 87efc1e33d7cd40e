"""CPU tier for the DXT5 -> ETC2 RGBA8 transcode (include/ic_amd.h, icamd_transcode_dxt5_to_etc2_rgba8).

* The block math of image-compression_amd/csrc/transcode5_block.h compiled for the host (tests/host_emul/transcode5_emul.cc,
  -DICAMD_HOST_EMULATION), byte for byte against the definition (tests/transcode5_oracle.py) on every block set.
* The palette-domain EAC search against encode_eac_alpha on the sixteen decoded alphas, block by block.
* The colour half against the DXT1 -> ETC1 transcode where the two agree (c0 > c1), and not where they must not.
* The C ABI's host-side surface: exports, the ICAMD_FALSE / ICAMD_ERR_ARG / ICAMD_OK cases, no CPU fall-back.
* (ref) the colour half pinned to the compiled reference itself.
* The new kernel compiles without scratch."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bc45_oracle as B
import ic_testlib as T
import transcode5_oracle as X

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
pkg = importlib.import_module("image-compression_amd")
KERNEL = "icamd_transcode_dxt5_to_etc2_rgba8_kernel"


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("transcode5") / "libtranscode5_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC,
                           "-I" + os.path.join(T.ROOT, "include"), "-o", so, os.path.join(EMUL_DIR, "transcode5_emul.cc")])
    L = ctypes.CDLL(so)
    L.transcode5_emul.restype = None
    L.transcode5_emul.argtypes = [T.vp, T.sz]
    for name in ("transcode5_emul_alpha_palette", "transcode5_emul_alpha_expanded"):
        getattr(L, name).restype = None
        getattr(L, name).argtypes = [T.sz, T.vp, T.vp]
    L.transcode5_emul_colour.restype = None
    L.transcode5_emul_colour.argtypes = [T.ci, T.sz, T.vp, T.vp]
    yield L
    T.assert_no_emul_violations(L, "test_transcode5_host")


def emul_transcode(L, blocks):
    b = np.frombuffer(bytes(blocks), np.uint8).copy()
    L.transcode5_emul(b.ctypes.data, b.size)
    return b.tobytes()


def emul_words(fn, words, *head):
    w = np.ascontiguousarray(words, np.uint8).reshape(-1, 8)
    out = np.zeros_like(w)
    fn(*head, w.shape[0], w.ctypes.data, out.ctypes.data)
    return out


# ---- the block sets are what they claim to be

def test_block_sets_cover_the_cases():
    sets = X.block_sets()
    rnd = sets["random"]
    assert rnd.shape[0] >= 4096
    c0 = rnd[:, 8].astype(int) | rnd[:, 9].astype(int) << 8
    c1 = rnd[:, 10].astype(int) | rnd[:, 11].astype(int) << 8
    assert (c0 <= c1).sum() > 1000 and (c0 > c1).sum() > 1000
    assert (rnd[:, 0] > rnd[:, 1]).sum() > 1000 and (rnd[:, 0] <= rnd[:, 1]).sum() > 1000
    for name in ("encoded_mixed", "encoded_noise", "encoded_saturated", "encoded_flat"):
        assert sets[name].shape[0] == 8 * 12
    assert (sets["a0_eq_a1"][:, 0] == sets["a0_eq_a1"][:, 1]).all()
    z = sets["zero_255_only"]
    assert (z[:, 0] <= z[:, 1]).all() and (X.unpack_codes(z) >= 6).all()
    dec = T.oracle_decode(T.DXT5, z.tobytes(), 4, 4 * z.shape[0]).reshape(4, -1, 4)[..., 3]
    assert set(np.unique(dec)) == {0, 255}
    s = X.unpack_codes(sets["single_code"])
    assert (s == s[:, :1]).all() and set(np.unique(s)) == set(range(8))
    inner = sets["inner_codes"]
    codes, pal = X.unpack_codes(inner), X.alpha_palette(inner)
    assert (codes >= 2).all()
    used = np.take_along_axis(pal, codes, axis=1)
    narrower = (used.min(axis=1) > pal.min(axis=1)) | (used.max(axis=1) < pal.max(axis=1))
    assert narrower.sum() > inner.shape[0] // 2  # lo / hi of the texels differ from the palette's extremes
    assert (X.unpack_codes(sets["flat_alpha"]) == 0).all()


# ---- the transcode against the definition

@pytest.mark.parametrize("name", sorted(X.block_sets()))
def test_emulated_transcode_matches_definition(emul, name):
    blocks = X.block_sets()[name]
    got = np.frombuffer(emul_transcode(emul, blocks.tobytes()), np.uint8).reshape(-1, 16)
    want = X.set_oracle(name)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (name, bad[:8], blocks[bad[:1]], got[bad[:1]], want[bad[:1]])


def test_tail_bytes_are_left_alone(emul):
    for n, tail in ((0, b""), (0, bytes(range(15))), (3, bytes(range(100, 108))), (5, bytes(range(1, 16)))):
        src, want = X.pool_blocks(n, tail)
        assert emul_transcode(emul, src) == want == X.oracle_transcode5(src), (n, len(tail))


def test_palette_search_equals_the_search_on_sixteen_alphas(emul):
    for name, blocks in sorted(X.block_sets().items()):
        words = blocks[:, :8]
        pal = emul_words(emul.transcode5_emul_alpha_palette, words)
        exp = emul_words(emul.transcode5_emul_alpha_expanded, words)
        bad = np.nonzero((pal != exp).any(axis=1))[0]
        assert bad.size == 0, (name, bad[:8], words[bad[:1]], pal[bad[:1]], exp[bad[:1]])
        assert ((pal[:, 1] >> 4) != 0).all(), name  # multiplier 0 is never written
        assert (pal == X.set_oracle(name)[:, :8]).all(), name


def test_colour_half_is_the_dxt1_transcode_only_for_four_colour_words(emul):
    blocks = np.concatenate([X.block_sets()[k] for k in ("random", "encoded_mixed", "encoded_saturated")], axis=0)
    colour = np.ascontiguousarray(blocks[:, 8:])
    c0 = colour[:, 0].astype(int) | colour[:, 1].astype(int) << 8
    c1 = colour[:, 2].astype(int) | colour[:, 3].astype(int) << 8
    four = c0 > c1
    assert four.sum() > 1000 and (~four).sum() > 1000
    got = np.frombuffer(emul_transcode(emul, blocks.tobytes()), np.uint8).reshape(-1, 16)[:, 8:]
    assert (got == emul_words(emul.transcode5_emul_colour, colour, 1)).all()
    dxt1 = np.frombuffer(T.oracle_transcode(colour.tobytes()), np.uint8).reshape(-1, 8)
    assert (emul_words(emul.transcode5_emul_colour, colour, 0) == dxt1).all()  # the existing path is what it was
    assert (got[four] == dxt1[four]).all()
    # DXT5 has no three-colour mode: the always-four palette is really exercised
    assert (got[~four] != dxt1[~four]).any(axis=1).sum() > 100


# ---- the C ABI's host-side surface (every check below returns before the GPU is touched)

def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    for name in ("icamd_transcode_dxt5_to_etc2_rgba8_device", "icamd_transcode_dxt5_to_etc2_rgba8"):
        assert hasattr(lib, name) and name in pkg.EXPORTS
    assert callable(pkg.transcode_dxt5_to_etc2_rgba8_host) and callable(pkg.transcode_dxt5_to_etc2_rgba8_device)


def test_argument_checks_come_before_the_device():
    lib = pkg.lib()
    aligned, off8, off1 = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x100008), ctypes.c_void_p(0x100001)  # never dereferenced
    assert lib.icamd_transcode_dxt5_to_etc2_rgba8_device(None, 64, None) == 1
    assert lib.icamd_transcode_dxt5_to_etc2_rgba8(None, 64) == 1
    for p in (off8, off1):
        assert lib.icamd_transcode_dxt5_to_etc2_rgba8_device(p, 64, None) == -4
        assert b"16-byte aligned" in lib.icamd_last_error()
        assert lib.icamd_transcode_dxt5_to_etc2_rgba8_device(p, 0, None) == -4  # alignment is checked before the size
    buf = np.arange(15, dtype=np.uint8)
    for n in (0, 15):
        assert lib.icamd_transcode_dxt5_to_etc2_rgba8_device(aligned, n, None) == 0
        assert lib.icamd_transcode_dxt5_to_etc2_rgba8(buf.ctypes.data, n) == 0
    assert (buf == np.arange(15)).all()


def test_a_real_call_needs_the_gpu_and_says_so():
    src, want = X.pool_blocks(5, b"\x01\x02\x03")
    buf = np.frombuffer(src, np.uint8).copy()
    rc = pkg.lib().icamd_transcode_dxt5_to_etc2_rgba8(buf.ctypes.data, buf.size)
    if pkg.lib().icamd_device_count() > 0:
        assert rc == 0 and buf.tobytes() == want
        return
    assert rc < 0 and b"no HIP device" in pkg.lib().icamd_last_error()
    assert buf.tobytes() == src  # no CPU result
    with pytest.raises(pkg.BackendError):
        pkg.transcode_dxt5_to_etc2_rgba8_host(src)


# ---- the colour half against the compiled reference (build container only)

@pytest.mark.ref
@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("h,w,gen", [(16, 24, "mixed"), (12, 20, "saturated")])
def test_colour_half_against_the_reference(emul, h, w, gen):
    img = B.image(gen, h, w, 4, index=h + w)
    dxt5 = T.oracle_encode(T.DXT5, img, h, w, 4)
    rgb = np.ascontiguousarray(T.oracle_decode(T.DXT5, dxt5, h, w).reshape(h, w, 4)[..., :3])
    ref = T.ref_compress(T.ETC, T.RGB, rgb, h, w, strategy=T.HEURISTIC)
    got = np.frombuffer(emul_transcode(emul, dxt5), np.uint8).reshape(-1, 16)[:, 8:].tobytes()
    assert got == ref


# ---- build check: the new kernel keeps everything in registers

def test_transcode5_kernel_uses_no_scratch(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path), "blockops_kernels.s")
    subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(T.ROOT, "include"),
                           "-I" + CSRC, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "blockops_kernels.hip")],
                          stderr=subprocess.DEVNULL)
    metas = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", open(out).read(), re.S):
        blk = m.group(0)
        metas[re.search(r"\.name:\s+(\S+)", blk).group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
    assert KERNEL in metas
    assert metas[KERNEL] == 0, "%s uses %d bytes of scratch" % (KERNEL, metas[KERNEL])
