"""CPU tier for the DXT1 -> ETC2 RGB8, BC4 -> EAC R11 and BC5 -> EAC RG11 transcodes (include/ic_amd.h,
icamd_transcode_dxt1_to_etc2_rgb8 / _bc4_to_eac_r11 / _bc5_to_eac_rg11).

* The block sets are what they claim to be, and the oracle alone takes both outcomes on them (planar and ETC1; a range that
  an unused palette entry would have changed).
* The block math of image-compression_amd/csrc/transcode_family_block.h compiled for the host
  (tests/host_emul/transcode_family_emul.cc, -DICAMD_HOST_EMULATION), byte for byte against the definition
  (tests/transcode_family_oracle.py) on every block set, and against the existing routines where the definition says so.
* The C ABI's host-side surface: exports, the ICAMD_FALSE / ICAMD_ERR_ARG / ICAMD_OK cases in the header's order, no CPU fall-back.
* The launch arithmetic of blockops_plan.h (tests/host_emul/transcode_family_plan_driver.cc).
* The three kernels compile without scratch."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import etc2_colour_oracle as C
import etc2_oracle as E
import ic_testlib as T
import transcode_family_oracle as X

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
pkg = importlib.import_module("image-compression_amd")
KIND_ID = {"dxt1": 0, "bc4": 1, "bc5": 2}
SYMBOL = {"dxt1": "icamd_transcode_dxt1_to_etc2_rgb8", "bc4": "icamd_transcode_bc4_to_eac_r11",
          "bc5": "icamd_transcode_bc5_to_eac_rg11"}
WRAPPER = {"dxt1": "transcode_dxt1_to_etc2_rgb8", "bc4": "transcode_bc4_to_eac_r11", "bc5": "transcode_bc5_to_eac_rg11"}
KERNELS = ["icamd_transcode_dxt1_to_etc2_rgb8_kernel", "icamd_transcode_bc4_to_eac_r11_kernel",
           "icamd_transcode_bc5_to_eac_rg11_kernel"]
ALL_SETS = [(k, name) for k in X.KINDS for name in sorted(X.block_sets(k))]


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("transcode_family") / "libtranscode_family_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC,
                           "-I" + os.path.join(T.ROOT, "include"), "-o", so, os.path.join(EMUL_DIR, "transcode_family_emul.cc")])
    L = ctypes.CDLL(so)
    L.transcode_family_emul.restype = None
    L.transcode_family_emul.argtypes = [T.ci, T.vp, T.sz]
    for name in ("transcode_family_emul_dxt1_to_etc1", "transcode_family_emul_dxt1_pixels", "transcode_family_emul_dxt5_alpha"):
        getattr(L, name).restype = None
        getattr(L, name).argtypes = [T.sz, T.vp, T.vp]
    yield L
    T.assert_no_emul_violations(L, "test_transcode_family_host")


def emul_transcode(L, kind, blocks):
    b = np.frombuffer(bytes(blocks), np.uint8).copy()
    L.transcode_family_emul(KIND_ID[kind], b.ctypes.data, b.size)
    return b.tobytes()


def emul_words(fn, words):
    w = np.ascontiguousarray(words, np.uint8).reshape(-1, 8)
    out = np.zeros_like(w)
    fn(w.shape[0], w.ctypes.data, out.ctypes.data)
    return out


# ---- the block sets are what they claim to be, and the oracle alone takes both outcomes

def test_dxt1_sets_cover_the_cases():
    sets = X.dxt1_sets()
    assert sets["random"].shape[0] >= 1 << 14
    c0, c1 = X.dxt1_endpoints(sets["random"])
    assert (c0 > c1).sum() > 4000 and (c0 < c1).sum() > 4000
    for name, rel in (("c0_gt_c1", np.greater), ("c0_lt_c1", np.less), ("c0_eq_c1", np.equal)):
        c0, c1 = X.dxt1_endpoints(sets[name])
        assert rel(c0, c1).all(), name
    s = X.dxt1_indices(sets["single_index"])
    assert (s == s[:, :1]).all() and set(np.unique(s)) == {0, 1, 2, 3}
    c0, c1 = X.dxt1_endpoints(sets["single_index"])
    assert (c0 > c1).any() and (c0 < c1).any()
    three = sets["three_colour_black"]
    c0, c1 = X.dxt1_endpoints(three)
    idx = X.dxt1_indices(three)
    assert (c0 < c1).all() and (idx == 3).any(axis=1).all() and (idx[:4] == 3).all()
    px = X.dxt1_pixels(three.tobytes()).reshape(4, -1, 4, 3).transpose(1, 0, 2, 3).reshape(-1, 16, 3)  # [block, 4 y + x, ch]
    assert (px[idx == 3] == 0).all()  # index 3 of the three-colour mode is black, as the DXT1 decoder decodes it
    assert sets["encoded_smooth"].shape[0] == 8 * 12 and sets["encoded_mixed"].shape[0] == 16 * 24


def test_the_dxt1_oracle_picks_planar_and_etc1():
    for name in ("encoded_smooth", "random"):
        planar = X.dxt1_choice(name)
        assert planar.any() and (~planar).any(), (name, int(planar.sum()), planar.size)
        got = X.set_oracle("dxt1", name)
        assert (C.modes(got[planar]) == C.PLANAR).all() and (C.modes(got[~planar]) <= C.DIFFERENTIAL).all()


def _eac_header_for_range(a, lo, hi):
    """The (table, multiplier, base) the EAC search of tests/etc2_oracle.py (eac_encode) settles on for the texels `a` [n, 16] when
    its candidates are laid around the range lo..hi [n] instead of the texels' own extremes: bytes 0 and 1 of the word (base;
    multiplier << 4 | table)."""
    a = np.asarray(a, np.int64)
    best = np.full(a.shape[0], np.iinfo(np.int64).max, np.int64)
    for t in range(16):
        span = int(E.SPAN[t])
        m0 = np.clip((2 * (hi - lo) + span) // (2 * span), 1, 15)
        for dm in (-1, 0, 1):
            m = np.clip(m0 + dm, 1, 15)
            b0 = (lo + hi + m + 1) >> 1
            for db in (-1, 0, 1):
                b = np.clip(b0 + db, 0, 255)
                vals = np.clip(b[:, None] + E.M[t][None, :] * m[:, None], 0, 255)
                e = np.abs(vals[:, None, :] - a[:, :, None]).min(axis=2)
                best = np.minimum(best, ((e * e).sum(axis=1) << 16) | (t << 12) | (m << 8) | b)
    return np.stack([best & 255, ((best >> 8) & 15) << 4 | ((best >> 12) & 15)], axis=1).astype(np.uint8)


def test_bc4_sets_cover_the_cases():
    sets = X.bc4_sets()
    rnd = sets["random"]
    assert rnd.shape[0] >= 1 << 14 and (rnd[:, 0] > rnd[:, 1]).sum() > 4000 and (rnd[:, 0] <= rnd[:, 1]).sum() > 4000
    assert (sets["a0_gt_a1"][:, 0] > sets["a0_gt_a1"][:, 1]).all()
    z = sets["a0_le_a1_0_255"]
    codes = X.bc4_codes(z)
    assert (z[:, 0] <= z[:, 1]).all() and (codes == 6).any(axis=1).all() and (codes == 7).any(axis=1).all()
    used = np.take_along_axis(X.bc4_palette(z), codes, axis=1)
    assert (used.min(axis=1) == 0).all() and (used.max(axis=1) == 255).all()
    assert (sets["a0_eq_a1"][:, 0] == sets["a0_eq_a1"][:, 1]).all()
    f = X.bc4_codes(sets["flat"])
    assert (f == f[:, :1]).all() and set(np.unique(f)) == set(range(8))
    assert (sets["flat"][:, 0] > sets["flat"][:, 1]).any() and (sets["flat"][:, 0] <= sets["flat"][:, 1]).any()
    for name in ("inner_codes", "inner_narrow"):
        w = sets[name]
        pal, codes = X.bc4_palette(w), X.bc4_codes(w)
        used = np.take_along_axis(pal, codes, axis=1)
        assert (used.min(axis=1) > pal.min(axis=1)).all() and (used.max(axis=1) < pal.max(axis=1)).all(), name


def test_an_unused_extreme_entry_would_change_the_bc4_oracles_word():
    changed = 0
    for name in ("inner_codes", "inner_narrow"):
        w = X.bc4_sets()[name]
        pal = X.bc4_palette(w)
        used = np.take_along_axis(pal, X.bc4_codes(w), axis=1)  # (the texels' order does not enter the search's sums)
        want = X.set_oracle("bc4", name)
        own = _eac_header_for_range(used, used.min(axis=1), used.max(axis=1))
        assert (own[:, 0] == want[:, 0]).all() and (own[:, 1] == want[:, 1]).all(), name  # the restated search is the oracle's
        widened = _eac_header_for_range(used, pal.min(axis=1), pal.max(axis=1))
        changed += int((widened != own).any(axis=1).sum())
    assert changed >= 1


def test_bc5_sets_pair_different_kinds():
    sets = X.bc5_sets()
    assert sets["random"].shape == (1 << 14, 16)
    k = sets["kinds_crossed"]
    assert ((k[:, 0] > k[:, 1]) != (k[:, 8] > k[:, 9])).sum() > 50  # the two channels of a block in different table modes


# ---- the block routines against the definition

@pytest.mark.parametrize("kind,name", ALL_SETS)
def test_emulated_transcode_matches_definition(emul, kind, name):
    blocks = X.block_sets(kind)[name]
    got = np.frombuffer(emul_transcode(emul, kind, blocks.tobytes()), np.uint8).reshape(-1, X.BLOCK[kind])
    want = X.set_oracle(kind, name)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (kind, name, bad[:8], blocks[bad[:1]], got[bad[:1]], want[bad[:1]])


@pytest.mark.parametrize("kind", X.KINDS)
def test_tail_bytes_are_left_alone(emul, kind):
    block = X.BLOCK[kind]
    for n, tail in ((0, b""), (0, bytes(range(block - 1))), (3, bytes(range(100, 100 + block // 2))), (5, bytes(range(1, block)))):
        src, want = X.pool_blocks(kind, n, tail)
        assert emul_transcode(emul, kind, src) == want == X.ORACLE[kind](src), (kind, n, len(tail))


# ---- ... and against the existing routines where the definition says so

def test_bc4_is_the_alpha_half_of_the_dxt5_transcoder(emul):
    for name, words in sorted(X.bc4_sets().items()):
        got = np.frombuffer(emul_transcode(emul, "bc4", words.tobytes()), np.uint8).reshape(-1, 8)
        assert (got == emul_words(emul.transcode_family_emul_dxt5_alpha, words)).all(), name
        assert ((got[:, 1] >> 4) != 0).all(), name  # multiplier 0 is never written


def test_bc5_is_bc4_on_each_half(emul):
    for name, blocks in sorted(X.bc5_sets().items()):
        got = np.frombuffer(emul_transcode(emul, "bc5", blocks.tobytes()), np.uint8).reshape(-1, 16)
        for half in (0, 8):
            one = np.ascontiguousarray(blocks[:, half:half + 8])
            want = np.frombuffer(emul_transcode(emul, "bc4", one.tobytes()), np.uint8).reshape(-1, 8)
            assert (got[:, half:half + 8] == want).all(), (name, half)


def test_dxt1_blocks_that_are_not_planar_are_the_etc1_transcode(emul):
    for name, blocks in sorted(X.dxt1_sets().items()):
        got = np.frombuffer(emul_transcode(emul, "dxt1", blocks.tobytes()), np.uint8).reshape(-1, 8)
        etc1 = emul_words(emul.transcode_family_emul_dxt1_to_etc1, blocks)
        assert (etc1 == np.frombuffer(T.oracle_transcode(blocks.tobytes()), np.uint8).reshape(-1, 8)).all(), name
        planar = C.modes(got) == C.PLANAR
        assert (planar == X.dxt1_choice(name)).all(), name
        assert (got[~planar] == etc1[~planar]).all(), name
        assert (C.modes(etc1) <= C.DIFFERENTIAL).all(), name  # E itself is never read as planar: `planar` above is the choice


def test_dxt1_plane_domain_form_equals_the_pixel_route(emul):
    for name, blocks in sorted(X.dxt1_sets().items()):
        got = np.frombuffer(emul_transcode(emul, "dxt1", blocks.tobytes()), np.uint8).reshape(-1, 8)
        assert (got == emul_words(emul.transcode_family_emul_dxt1_pixels, blocks)).all(), name


# ---- the C ABI's host-side surface (every check below returns before the GPU is touched)

def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    for kind in X.KINDS:
        for name in (SYMBOL[kind] + "_device", SYMBOL[kind]):
            assert hasattr(lib, name) and name in pkg.EXPORTS, name
        assert callable(getattr(pkg, WRAPPER[kind] + "_host")) and callable(getattr(pkg, WRAPPER[kind] + "_device"))


@pytest.mark.parametrize("kind", X.KINDS)
def test_argument_checks_come_before_the_device(kind):
    lib = pkg.lib()
    block = X.BLOCK[kind]
    device_form, host_form = getattr(lib, SYMBOL[kind] + "_device"), getattr(lib, SYMBOL[kind])
    aligned = ctypes.c_void_p(0x100000)  # never dereferenced
    misaligned = [ctypes.c_void_p(0x100000 + k) for k in ((1, 4) if block == 8 else (1, 4, 8))]
    # NULL first
    assert device_form(None, 64, None) == 1 and host_form(None, 64) == 1
    assert device_form(None, 0, None) == 1 and host_form(None, 0) == 1
    # then the alignment, before the size
    for p in misaligned:
        assert device_form(p, 64, None) == -4
        assert (b"%d-byte aligned" % block) in lib.icamd_last_error()
        assert device_form(p, 0, None) == -4
    # then fewer bytes than a block: nothing to do, with or without a device
    buf = np.arange(block - 1, dtype=np.uint8)
    for n in (0, block - 1):
        assert device_form(aligned, n, None) == 0
        assert host_form(buf.ctypes.data, n) == 0
    assert (buf == np.arange(block - 1)).all()


@pytest.mark.parametrize("kind", X.KINDS)
def test_a_real_call_needs_the_gpu_and_says_so(kind):
    src, want = X.pool_blocks(kind, 5, b"\x01\x02\x03")
    buf = np.frombuffer(src, np.uint8).copy()
    lib = pkg.lib()
    rc = getattr(lib, SYMBOL[kind])(buf.ctypes.data, buf.size)
    if lib.icamd_device_count() > 0:
        assert rc == 0 and buf.tobytes() == want
        return
    assert rc == -1 and b"no HIP device" in lib.icamd_last_error()  # ICAMD_ERR_NO_DEVICE, and only after validation
    assert buf.tobytes() == src  # no CPU result
    assert getattr(lib, SYMBOL[kind] + "_device")(ctypes.c_void_p(0x100000), 64, None) == -1
    with pytest.raises(pkg.BackendError):
        getattr(pkg, WRAPPER[kind] + "_host")(src)


# ---- the launch arithmetic

def test_plan_cuts_buffers_into_32_bit_launches(tmp_path):
    exe = os.path.join(str(tmp_path), "transcode_family_plan_driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + CSRC, "-o", exe,
                           os.path.join(EMUL_DIR, "transcode_family_plan_driver.cc")])
    lines = subprocess.check_output([exe]).decode().splitlines()
    chunk = 1 << 30  # blocks per launch: a 32-bit block index, and at most 2^24 one-wave workgroups
    cases, i = {}, 0
    while i < len(lines):
        assert lines[i].startswith("= ")
        n_bytes, block, lanes, blocks, launches = (int(v) for v in lines[i].split()[1:])
        shown = min(launches, 4)
        cases[(n_bytes, block, lanes)] = (blocks, launches, [tuple(int(v) for v in ln.split()) for ln in lines[i + 1:i + 1 + shown]])
        i += 1 + shown
    assert len(cases) == 30
    for block, lanes in ((8, 256), (8, 64), (16, 64)):
        for n_bytes in (0, block - 1, block, block + 1, chunk * block - 1, chunk * block, chunk * block + block - 1,
                        chunk * block + block, 1 << 40, (1 << 40) + 7):
            blocks, launches, shown = cases[(n_bytes, block, lanes)]
            assert blocks == n_bytes // block and launches == -(-blocks // chunk), (n_bytes, block)
            which = range(launches) if launches <= 4 else (0, 1, launches - 2, launches - 1)
            assert len(shown) == len(list(which))
            for k, (idx, first, offset, count, grid_x, got_lanes) in zip(which, shown):
                want_count = min(chunk, blocks - k * chunk)
                assert (idx, first, offset, count) == (k, k * chunk, k * chunk * block, want_count), (n_bytes, block, k)
                assert got_lanes == lanes and grid_x == -(-want_count // lanes)
                assert 0 < count <= chunk and grid_x * lanes < 1 << 31  # the kernel's 32-bit index never wraps
    # the cases by name: nothing, one block, exactly one chunk, one chunk plus one block, 2^40 bytes
    assert cases[(0, 8, 64)][:2] == (0, 0) and cases[(8, 8, 64)][:2] == (1, 1) and cases[(16, 16, 64)][2] == [(0, 0, 0, 1, 1, 64)]
    assert cases[(chunk * 8, 8, 256)][:2] == (chunk, 1) and cases[(chunk * 8 + 8, 8, 256)][:2] == (chunk + 1, 2)
    assert cases[(chunk * 8 + 8, 8, 256)][2][1] == (1, chunk, chunk * 8, 1, 1, 256)
    assert cases[(1 << 40, 8, 64)][:2] == (1 << 37, 128) and cases[(1 << 40, 16, 64)][:2] == (1 << 36, 64)


# ---- build check: the new kernels keep everything in registers

def test_transcode_family_kernels_use_no_scratch(tmp_path):
    import test_isa_guards as G
    text = G._asm("blockops_kernels.hip", tmp_path)
    for kernel in KERNELS:
        meta = G._kernel_meta(text, kernel)
        assert meta["scratch"] == 0, "%s uses %d bytes of scratch" % (kernel, meta["scratch"])
        assert meta["lds"] == 0, kernel
