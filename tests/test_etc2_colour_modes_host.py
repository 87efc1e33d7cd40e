"""CPU tier for icamd_encode_etc2_colour_device: planar, T and H colour words for ETC2 RGBA8 and ETC2 RGB8A1 (include/ic_amd.h;
DESIGN.md 3.19).

* The fixtures have the properties the definition gives them, asserted on the numpy definition (tests/etc2_a1_th_oracle.py).
* The block math of image-compression_amd/csrc/etc2_a1_th_block.h, the ETC2 RGBA8 chaining and the block walk of both passes
  compiled for the host (tests/host_emul/etc2_a1_th_emul.cc, -DICAMD_HOST_EMULATION), bit-exact against the definition: fixtures,
  random blocks with random masks, constructed corner blocks.
* The definition's output checked through the decoders' oracles alone (transparency mask, error, mode).
* The C ABI's host-side surface of icamd_encode_etc2_colour_device / icamd_etc2_colour_kernel_name, and the Python function.

The fixture tests and test_output_of_the_definition_checked_independently run no product code: they pin the DEFINITION (the numpy
oracle every other test here and in the GPU tier compares against).  The host-twin, ABI and keyword tests are the ones that fail
without the feature."""
import ctypes
import functools
import importlib
import os
import subprocess

import numpy as np
import pytest

import etc2_a1_oracle as A
import etc2_a1_th_oracle as M
import etc2_colour_oracle as C
import etc2_oracle as E2
import etc2_th_oracle as H
import ic_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
pkg = importlib.import_module("image-compression_amd")
OK, FALSE, ERR_NO_DEVICE, ERR_ARG = 0, 1, -1, -4
RGBA8, RGB8, RGB8A1 = M.ETC2_RGBA8, M.ETC2_RGB8, M.ETC2_RGB8A1
COMBOS = {(p, k) for p in (M.PART_L, M.PART_C) for k in (M.KIND_T_AB, M.KIND_T_BA, M.KIND_H)}
FIXTURES = {"cut": M.edges_cut, "blobs": M.edges_blobs, "noise": M.edges_noise, "mixed": M.mixed}


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("etc2cm") / "libetc2_a1_th_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC,
                           "-I" + os.path.join(T.ROOT, "include"), "-o", so, os.path.join(EMUL_DIR, "etc2_a1_th_emul.cc")])
    L = ctypes.CDLL(so)
    L.etc2cm_emul_encode.restype = ctypes.c_int
    L.etc2cm_emul_encode.argtypes = [T.ci, T.ci, T.ci, T.u32, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp]
    L.etc2cm_emul_masked_search.restype = None
    L.etc2cm_emul_masked_search.argtypes = [T.u32, T.vp, T.vp]
    yield L
    T.assert_no_emul_violations(L, "test_etc2_colour_modes_host")


def emul_encode(L, codec, flat, h, w, strategy=2, modes=M.COLOUR_PLANAR_TH, gh=None, gw=None, stride=None):
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    out = np.zeros(((gh + 3) // 4) * ((gw + 3) // 4) * (16 if codec == RGBA8 else 8), np.uint8)
    src = np.ascontiguousarray(flat, dtype=np.uint8).reshape(-1)
    assert L.etc2cm_emul_encode(codec, strategy, modes, h, w, gh, gw, w * 4 if stride is None else stride, src.ctypes.data,
                                out.ctypes.data)
    return out.tobytes()


def strip(tex):
    """[n, 4(y), 4(x), 4] blocks -> the 4 x 4n RGBA image that holds them side by side."""
    tex = np.asarray(tex, np.uint8)
    return np.ascontiguousarray(tex.transpose(1, 0, 2, 3).reshape(4, 4 * tex.shape[0], 4))


@functools.lru_cache(maxsize=None)
def fixture_image(name):
    img = FIXTURES[name]()
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def want(name, strategy=T.SMALLER_ERROR):
    """(bytes, choice) of the RGB8A1 definition for a 64 x 64 fixture; computed once, never written to."""
    out, choice = M.oracle_encode(fixture_image(name), 64, 64, 0, strategy, return_choice=True)
    choice.setflags(write=False)
    return out, choice


def words(b):
    return np.frombuffer(b, np.uint8).reshape(-1, 8)


# ---- the fixtures, on the definition

def test_fixtures_take_every_kind_partition_and_h_order_in_blocks_with_transparency():
    choice = np.concatenate([want(name)[1] for name in sorted(FIXTURES)])
    out = np.concatenate([words(want(name)[0]) for name in sorted(FIXTURES)])
    mixed = choice[:, M.COL_CLASS] == M.CLASS_MIXED
    ch = M.changed(choice)
    assert (mixed & ~ch).sum() >= 16 and (mixed & ch).sum() >= 16      # blocks that keep W, blocks that change
    assert {tuple(c) for c in choice[mixed & ch][:, M.COL_PART:M.COL_DI].tolist()} == COMBOS  # both partitions, all three kinds
    m = A.modes(out[mixed & ch])
    assert (m == A.T_MODE).any() and (m == A.H_MODE).any() and ((m == A.T_MODE) | (m == A.H_MODE)).all()
    h = mixed & ch & (choice[:, M.COL_KIND] == M.KIND_H)
    assert set(choice[h][:, M.COL_SWAPPED].tolist()) == {0, 1}           # both H storage orders
    for parity in (0, 1):                                                 # ... at even and at odd di
        assert set(choice[h & (choice[:, M.COL_DI] % 2 == parity)][:, M.COL_SWAPPED].tolist()) == {0, 1}
    full = choice[:, M.COL_CLASS] == M.CLASS_OPAQUE
    assert (full & ch).sum() >= 16                                        # class 2 blocks that change
    assert (A.opaque_bit(out[full & ch]) == 1).all() and (A.opaque_bit(out[mixed]) == 0).all()


@pytest.mark.parametrize("name", ["cut", "blobs", "noise"])
def test_each_mask_fixture_has_blocks_with_transparency_that_change(name):
    _, choice = want(name)
    mixed = choice[:, M.COL_CLASS] == M.CLASS_MIXED
    assert (mixed & M.changed(choice)).sum() >= 8, name
    if name == "cut":  # the cut runs through block column 5: columns 20, 21 transparent, 22, 23 opaque
        assert (np.flatnonzero(mixed) % 16 == 5).all() and mixed.sum() == 16


@pytest.mark.parametrize("strategy", C.STRATEGIES)
def test_mixed_fixture_holds_every_class_changed_and_kept_in_every_wave(strategy):
    kinds = M.wave_kinds(fixture_image("mixed"), strategy=strategy)
    assert len(kinds) == 4 and all(min(k) >= 4 for k in kinds), dict(zip(M.WAVE_KINDS, zip(*kinds)))


# ---- host twin against the definition

@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_host_twin_on_the_fixtures_rgb8a1(emul, name):
    img = fixture_image(name)
    for strategy in C.STRATEGIES + (7,):  # (out of range: kSmallerError)
        st = strategy if strategy < 4 else T.SMALLER_ERROR
        assert emul_encode(emul, RGB8A1, img, 64, 64, strategy) == want(name, st)[0], (name, strategy)
        for modes in (M.COLOUR_DEFAULT, M.COLOUR_PLANAR):
            assert emul_encode(emul, RGB8A1, img, 64, 64, strategy, modes=modes) == A.oracle_encode(img, 64, 64, 0, st)


@functools.lru_cache(maxsize=None)
def alpha_words(name):
    return E2.eac_encode(E2.block_alphas(fixture_image(name)[..., 3], 64, 64, 64, 64))


@pytest.mark.parametrize("modes", [M.COLOUR_PLANAR, M.COLOUR_PLANAR_TH])
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_host_twin_on_the_fixtures_rgba8(emul, name, modes):
    img = fixture_image(name)
    for strategy in C.STRATEGIES:
        colour = (C.oracle_encode if modes == M.COLOUR_PLANAR else H.oracle_encode)(img, 64, 64, 4, 0, strategy)
        expect = np.concatenate([alpha_words(name), words(colour)], axis=1).tobytes()
        assert expect == M.oracle_encode_rgba8(img, 64, 64, 0, strategy, modes=modes, alpha_words=alpha_words(name))
        got = emul_encode(emul, RGBA8, img, 64, 64, strategy, modes=modes)
        assert got == expect, (name, modes, strategy)
        if modes == M.COLOUR_PLANAR_TH:
            m = C.modes(np.frombuffer(got, np.uint8).reshape(-1, 16)[:, 8:])
            assert (m == C.T_MODE).any() and (m == C.H_MODE).any() and (m == C.PLANAR).any(), (name, strategy)
    assert emul_encode(emul, RGBA8, img, 64, 64, modes=M.COLOUR_DEFAULT) == E2.oracle_encode(img, 64, 64, alpha_words=alpha_words(name))


def test_host_twin_padded_grid_and_row_padding(emul):
    img = M.edges_blobs(6, 61, 59)
    assert emul_encode(emul, RGB8A1, img, 61, 59, gh=64, gw=64) == M.oracle_encode(img, 61, 59, gh=64, gw=64)
    assert emul_encode(emul, RGBA8, img, 61, 59, gh=64, gw=64) == M.oracle_encode_rgba8(img, 61, 59, gh=64, gw=64)
    flat = T.with_row_padding(img, 5)
    assert emul_encode(emul, RGB8A1, flat, 61, 59, stride=59 * 4 + 5) == M.oracle_encode(img, 61, 59)
    assert emul_encode(emul, RGBA8, flat, 61, 59, stride=59 * 4 + 5) == M.oracle_encode_rgba8(img, 61, 59)


def random_blocks():
    """20 480 blocks with random masks: noise, two noisy colours under a random mask, two close colours, low-contrast noise;
    the alpha per texel random with a per-block bias, so that n runs over 0..16."""
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9910))
    n = 5120
    noise = g.integers(0, 256, (n, 4, 4, 3))
    mask = g.integers(0, 2, (2 * n, 4, 4, 1)).astype(bool)
    c1, c2 = g.integers(0, 256, (2 * n, 1, 1, 3)), g.integers(0, 256, (2 * n, 1, 1, 3))
    c2[n:] = c1[n:] + g.integers(-20, 21, (n, 1, 1, 3))  # close colours: codes that collide, partitions that coincide
    two = np.where(mask, c1, c2) + g.integers(-4, 5, (2 * n, 4, 4, 3))
    low = g.integers(0, 256, (n, 1, 1, 3)) + g.integers(-9, 10, (n, 4, 4, 3))
    rgb = np.clip(np.concatenate([noise, two, low]), 0, 255)
    bias = g.integers(0, 256, (4 * n, 1, 1))
    alpha = np.where(g.integers(0, 256, (4 * n, 4, 4)) < bias, 255, g.integers(0, 128, (4 * n, 4, 4)))
    return np.concatenate([rgb, alpha[..., None]], axis=-1).astype(np.uint8)


def corner_blocks():
    """Constructed blocks, each (4, 4, 4) RGBA: the corner cases of the masked search."""
    blocks = []

    def block(fill, transparent=(), **texels):
        b = np.empty((4, 4, 4), np.int64)
        b[..., :3], b[..., 3] = fill, 255
        for key, colour in texels.items():
            b[int(key[1]), int(key[2]), :3] = colour
        for y, x in transparent:
            b[y, x, 3] = 0
        blocks.append(b)
        return b

    everything = [(y, x) for y in range(4) for x in range(4)]
    block((20, 30, 40), transparent=everything[1:])                                   # n = 1: must be W
    block((200, 30, 40), transparent=everything[:15])                                 # n = 1, the last texel
    block((20, 30, 40), transparent=everything[2:], t01=(250, 240, 230))              # n = 2: one-texel clusters
    block((20, 30, 40), transparent=everything[1:15], t33=(250, 30, 40))              # n = 2, far apart in the block
    block((100, 100, 100), transparent=[(3, 3)], t00=(104, 104, 104))                 # equal cluster codes: dropped
    block((100, 100, 100), transparent=[(0, 3)], t00=(108, 100, 100), t11=(108, 100, 100))
    block((0, 0, 0), transparent=[(2, 2)], t00=(255, 255, 255), t01=(255, 255, 255))  # paints clamp at both ends
    block((5, 5, 5), transparent=[(3, 0)], t00=(250, 250, 250), t01=(0, 0, 0), t10=(255, 255, 255))
    block((255, 255, 255), transparent=[(1, 1), (1, 2)], t30=(0, 0, 0))
    # texels midway between paints: C1 = 0, C2 = 136 (codes 0 and 8); a texel equidistant from paints 1 and 3 (it is C2 itself:
    # index 2 is not allowed), one from paints 0 and 1, for every distance
    for d in C.DIST:
        b = np.zeros((4, 4, 4), np.int64)
        b[..., 3] = 255
        b[:, 2:, :3] = 136
        b[0, 2, :3] = 136 + d
        b[1, 2, :3] = 136 - d
        b[2, 2, :3] = 136                       # between paints 1 and 3
        b[3, 2, :3] = (136 + d) // 2            # between paints 0 and 1 of T(a, b)
        b[0, 0, :3] = 68
        b[3, 3, 3] = 0
        blocks.append(b)
    # two flat halves under a hole: candidates tie at several distances; the earliest must win.  Both orders of the colours:
    # H with a >= b and with a < b, at even and odd di
    for a, b2 in (((17, 17, 17), (238, 238, 238)), ((238, 238, 238), (17, 17, 17)), ((0, 0, 0), (255, 255, 255)),
                  ((51, 102, 153), (153, 102, 51)), ((153, 102, 51), (51, 102, 153)), ((34, 34, 34), (40, 34, 34)),
                  ((3, 3, 3), (20, 20, 20)), ((20, 14, 17), (3, 9, 6)), ((200, 40, 30), (30, 60, 200))):
        for split in (1, 2, 3):
            for hole in ((0, 0), (3, 3), (1, 2)):
                blk = np.empty((4, 4, 4), np.int64)
                blk[..., 3] = 255
                blk[:, :split, :3], blk[:, split:, :3] = a, b2
                blk[hole[0], hole[1], 3] = 0
                blocks.append(blk)
                blocks.append(blk.transpose(1, 0, 2).copy())
    # H-friendly blocks: four levels a +- d, b - d around two colours in both orders
    # (the darker cluster is a: (170, 51, 85) is a >= b against (85, 153, 170), (68, 68, 68) is a < b against (187, 187, 187);
    # the three levels sit on the colour that must be stored first)
    for d in (6, 11, 16, 23, 41):
        for ca, cb in (((68, 68, 68), (187, 187, 187)), ((187, 187, 187), (68, 68, 68)), ((170, 51, 85), (85, 153, 170)),
                       ((85, 153, 170), (170, 51, 85))):
            blk = np.empty((4, 4, 4), np.int64)
            blk[..., 3] = 255
            ca, cb = np.array(ca), np.array(cb)
            blk[0, :, :3], blk[1, :, :3], blk[2, :, :3], blk[3, :, :3] = ca + d, ca - d, cb - d, cb - d
            blk[0, 0, 3] = blk[2, 1, 3] = 0
            blocks.append(blk)
    block((90, 160, 40), transparent=[(0, 0)])                                        # flat: no partition survives
    block((90, 165, 41), transparent=[(0, 0)])                                        # err(W) = 0
    block((90, 165, 41), transparent=[(0, 0)], t33=(98, 173, 49))                     # err(W) = 0 with two colours (+b of table 0)
    block((20, 30, 40), transparent=[(0, 0)], t12=(250, 240, 230), t21=(120, 130, 140))   # only texel 0 transparent
    block((20, 30, 40), transparent=[(3, 3)], t12=(250, 240, 230), t21=(120, 130, 140))   # only texel 15 transparent
    # equal luminance (partition L dropped) and equal ranges (the channel tie goes to R, then G)
    block((200, 50, 100), transparent=[(1, 0)], t00=(100, 100, 100), t22=(100, 100, 100))
    block((10, 10, 10), transparent=[(1, 0)], t00=(60, 60, 60))
    block((10, 10, 10), transparent=[(1, 0)], t00=(10, 60, 60))
    block((10, 10, 10), transparent=[(1, 0)], t00=(10, 10, 60), t01=(10, 60, 10))
    # an extreme colour hidden under a transparent texel must not move the partitions
    b = block((10, 10, 10), transparent=[(1, 0)], t00=(60, 60, 60))
    b[1, 0, :3] = 255
    return np.clip(np.stack(blocks), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def block_cases():
    tex = np.concatenate([corner_blocks(), random_blocks()])
    img = strip(tex)
    n = tex.shape[0]
    out, choice = M.oracle_encode(img, 4, 4 * n, return_choice=True)
    base = A.oracle_encode(img, 4, 4 * n)
    return tex, img, out, choice, base


def test_corner_blocks_are_what_they_are_built_to_be():
    tex, img, out, choice, base = block_cases()
    k = corner_blocks().shape[0]
    assert (choice[:k, M.COL_CLASS] == M.CLASS_MIXED).all()
    got, w = words(out)[:k], words(base)[:k]
    opq = tex[:k, ..., 3] >= 128
    n_o = opq.sum(axis=(1, 2))
    assert (n_o[:2] == 1).all() and (got[:2] == w[:2]).all()          # n = 1 is W
    assert (n_o[2:4] == 2).all() and M.changed(choice[2:4]).all()      # n = 2: one-texel clusters, and they win
    err_w = M.sse_opaque(tex[:k, ..., :3], opq, w)
    assert (err_w == 0).sum() >= 2 and (got[err_w == 0] == w[err_w == 0]).all()
    assert not opq[-7, 0, 0] and opq[-7].sum() == 15 and not opq[-6, 3, 3] and opq[-6].sum() == 15  # texel 0 / texel 15 only
    assert M.changed(choice[k - 7:k - 5]).all()
    h = M.changed(choice[:k]) & (choice[:k, M.COL_KIND] == M.KIND_H)
    for parity in (0, 1):
        assert set(choice[:k][h & (choice[:k, M.COL_DI] % 2 == parity)][:, M.COL_SWAPPED].tolist()) == {0, 1}
    # the hidden extreme colour changes nothing: the same word as the block before it
    assert (got[-1] == got[-4]).all()


def test_host_twin_on_random_and_corner_blocks(emul):
    tex, img, out, choice, base = block_cases()
    n = tex.shape[0]
    assert n >= 20000
    assert (A.block_texels(img, 4, 4 * n, 4, 4 * n) == tex).all()
    cls, ch = choice[:, M.COL_CLASS], M.changed(choice)
    for c in (M.CLASS_CLEAR, M.CLASS_OPAQUE, M.CLASS_MIXED):
        assert (cls == c).sum() >= 200
    mixed = cls == M.CLASS_MIXED
    assert 0.2 < ch[mixed].mean() < 0.98  # both outcomes in numbers
    got = emul_encode(emul, RGB8A1, img, 4, 4 * n)
    bad = np.flatnonzero((words(got) != words(out)).any(axis=1))
    assert bad.size == 0, (bad[:8], choice[bad[:8]])
    assert emul_encode(emul, RGB8A1, img, 4, 4 * n, modes=M.COLOUR_PLANAR) == base
    for modes in (M.COLOUR_PLANAR, M.COLOUR_PLANAR_TH):
        assert emul_encode(emul, RGBA8, img, 4, 4 * n, modes=modes) == M.oracle_encode_rgba8(img, 4, 4 * n, modes=modes), modes


def test_masked_search_key_is_the_definitions_error_and_order(emul):
    tex, _, _, choice, _ = block_cases()
    tex = tex[choice[:, M.COL_CLASS] == M.CLASS_MIXED]
    n = tex.shape[0]
    _, err, ch = M.masked_search(tex[..., :3], tex[..., 3] >= 128)
    keys = np.zeros(n, np.uint32)
    flat = np.ascontiguousarray(tex.reshape(n, 64))
    emul.etc2cm_emul_masked_search(n, flat.ctypes.data, keys.ctypes.data)
    none = err == M.NO_ERROR
    assert none.any() and (keys[none] == 0xffffffff).all()
    order = 24 * ch[:, 0] + 8 * ch[:, 1] + ch[:, 2]
    assert (keys[~none].astype(np.int64) == (err[~none] << 6 | order[~none])).all()


# ---- the definition's output, through the decoders' oracles alone

def test_output_of_the_definition_checked_independently():
    tex, img, out, choice, base = block_cases()
    got, w = words(out), words(base)
    ch = M.changed(choice)
    cls = choice[:, M.COL_CLASS]
    assert ((got != w).any(axis=1) == ch).all()                     # unchanged blocks are W byte for byte
    assert not ch[cls == M.CLASS_CLEAR].any()
    dec, dec_w = A.decode_blocks(got), A.decode_blocks(w)
    opq = tex[..., 3] >= 128
    assert ((dec[..., 3] == 255) == opq).all() and ((dec_w[..., 3] == 255) == opq).all()  # no texel gained or lost
    assert ((dec[..., 3] == 0) == ~opq).all()
    err_out, err_w = M.sse_opaque(tex[..., :3], opq, got), M.sse_opaque(tex[..., :3], opq, w)
    assert (err_out[ch] < err_w[ch]).all() and (err_out[~ch] == err_w[~ch]).all()
    m = A.modes(got[ch])
    assert (m == np.where(choice[ch][:, M.COL_KIND] == M.KIND_H, A.H_MODE, A.T_MODE)).all()
    assert (A.opaque_bit(got[ch]) == (cls[ch] == M.CLASS_OPAQUE)).all()
    mixed = cls == M.CLASS_MIXED
    _, claimed, _ = M.masked_search(tex[mixed][..., :3], opq[mixed])
    assert (err_out[mixed][ch[mixed]] == claimed[ch[mixed]]).all()   # the decoder renders what the search counted
    assert (claimed[~ch[mixed]] >= err_w[mixed][~ch[mixed]]).all()
    # the stored distance index is the intended one (H: its lowest bit is the order of the stored colours)
    hi = got[ch].astype(np.int64)
    t_di = ((hi[:, 3] >> 2) & 3) << 1 | (hi[:, 3] & 1)
    is_t = m == A.T_MODE
    assert (t_di[is_t] == choice[ch][is_t, M.COL_DI]).all()
    h_top = ((hi[:, 3] >> 2) & 1) << 2 | (hi[:, 3] & 1) << 1
    assert (h_top[~is_t] == (choice[ch][~is_t, M.COL_DI] & 6)).all()


def test_rgba8_definition_keeps_alpha_and_never_adds_error():
    for name in sorted(FIXTURES):
        img = fixture_image(name)
        tex = C.block_texels(img, 64, 64, 64, 64)[..., :3]
        base = np.frombuffer(E2.oracle_encode(img, 64, 64, alpha_words=alpha_words(name)), np.uint8).reshape(-1, 16)
        last = C.sse(tex, C.decode_blocks(base[:, 8:]))
        for modes in (M.COLOUR_PLANAR, M.COLOUR_PLANAR_TH):
            got = np.frombuffer(M.oracle_encode_rgba8(img, 64, 64, modes=modes, alpha_words=alpha_words(name)), np.uint8).reshape(-1, 16)
            assert (got[:, :8] == base[:, :8]).all()
            err = C.sse(tex, C.decode_blocks(got[:, 8:]))
            assert (err <= last).all() and err.sum() < last.sum(), (name, modes)
            last = err
        # alpha never enters the colour choice
        other = img.copy()
        other[..., 3] = 255 - other[..., 3]
        again = np.frombuffer(M.oracle_encode_rgba8(other, 64, 64), np.uint8).reshape(-1, 16)
        assert (again[:, 8:] == got[:, 8:]).all()


# ---- the C ABI's host-side surface (every check below returns before the GPU is touched)

def _call(lib, codec=RGBA8, strategy=2, modes=2, comps=4, swap=0, h=8, w=8, gh=8, gw=8, stride=None, n=1, src=16, dst=16):
    stride = w * comps if stride is None else stride
    return lib.icamd_encode_etc2_colour_device(codec, strategy, modes, comps, swap, h, w, gh, gw, stride, n, 0, 0,
                                               ctypes.c_void_p(src) if src else None, ctypes.c_void_p(dst) if dst else None, None)


@pytest.mark.parametrize("codec", [RGBA8, RGB8, RGB8A1])
def test_argument_errors(codec):
    lib = pkg.lib()  # (the pointers are never dereferenced: the arguments are refused first)
    for modes in (0, 1, 2):
        assert _call(lib, codec, modes=modes, src=0) == FALSE and _call(lib, codec, modes=modes, dst=0) == FALSE
        assert _call(lib, codec, modes=modes, h=0) == FALSE and _call(lib, codec, modes=modes, w=0) == FALSE
        assert _call(lib, codec, modes=modes, h=0, comps=7) == FALSE       # a zero size comes before every argument error
        assert _call(lib, codec, modes=modes, n=0) == OK
        assert _call(lib, codec, modes=modes, n=0, stride=31) == OK        # an empty batch comes before the stride
        assert _call(lib, codec, modes=modes, stride=31) == ERR_ARG
        for comps in (1, 2, 5):
            assert _call(lib, codec, modes=modes, comps=comps) == ERR_ARG and _call(lib, codec, modes=modes, comps=comps, n=0) == ERR_ARG
        want3 = OK if codec == RGB8 else ERR_ARG
        assert _call(lib, codec, modes=modes, comps=3, n=0) == want3
        if codec == RGB8:
            assert _call(lib, codec, modes=modes, comps=3, stride=23) == ERR_ARG
    for modes in (-1, 3, 4):
        assert _call(lib, codec, modes=modes) == ERR_ARG and _call(lib, codec, modes=modes, n=0) == ERR_ARG


def test_other_codecs_are_refused():
    lib = pkg.lib()
    for codec in list(range(-1, 16)) + [17, 19, 20, 22, 23]:
        for modes in (0, 1, 2):
            assert _call(lib, codec, modes=modes) == ERR_ARG and _call(lib, codec, modes=modes, n=0) == ERR_ARG, codec
            assert _call(lib, codec, modes=modes, h=0) == FALSE


def test_valid_arguments_fail_loudly_without_a_device():
    if pkg.lib().icamd_device_count() > 0:
        pytest.skip("a device is present: the GPU tier runs this call")
    for codec in (RGBA8, RGB8, RGB8A1):
        for modes in (0, 1, 2):
            assert _call(pkg.lib(), codec, modes=modes) == ERR_NO_DEVICE


def test_kernel_names_and_constants():
    assert (pkg.ETC2_COLOUR_DEFAULT, pkg.ETC2_COLOUR_PLANAR, pkg.ETC2_COLOUR_PLANAR_TH) == (0, 1, 2)
    assert (M.COLOUR_DEFAULT, M.COLOUR_PLANAR, M.COLOUR_PLANAR_TH) == (0, 1, 2)
    name = pkg.etc2_colour_kernel_name
    assert name(RGBA8, 4, 1) == "icamd_etc2_rgba8_planar_kernel"
    assert name(RGBA8, 4, 2) == "icamd_etc2_rgba8_planar_th_kernel"
    assert name(RGB8A1, 4, 2) == "icamd_etc2_a1_th_kernel"
    assert name(RGB8A1, 4, 1) == pkg.kernel_name(RGB8A1, 4) != ""       # PLANAR is icamd_encode_device
    for comps in (3, 4):
        assert name(RGB8, comps, 1) == pkg.kernel_name(RGB8, comps) != ""
        assert name(RGB8, comps, 2) == pkg.etc2_kernel_name(RGB8, comps, pkg.ETC2_MODES_TH) != ""
    for codec in list(range(0, 7)) + [16, 17, 18, 19, 20, 21, 22]:
        for comps in (1, 2, 3, 4, 5):
            assert name(codec, comps, 0) == pkg.kernel_name(codec, comps), (codec, comps)
    for codec, comps, modes in ((RGBA8, 3, 1), (RGBA8, 3, 2), (RGB8A1, 3, 2), (RGB8A1, 3, 1), (RGB8, 2, 1), (RGB8, 5, 2),
                                (RGBA8, 4, 3), (RGBA8, 4, -1), (RGB8A1, 4, 3), (RGB8, 3, 3), (2, 3, 1), (2, 4, 2), (17, 4, 2),
                                (19, 4, 1), (20, 4, 2)):
        assert name(codec, comps, modes) == "", (codec, comps, modes)
    assert "icamd_encode_etc2_colour_device" in pkg.EXPORTS and "icamd_etc2_colour_kernel_name" in pkg.EXPORTS


def test_python_function_reaches_the_new_entry_point(monkeypatch):
    calls = []
    real = pkg.lib()

    class Tensor:  # what the function touches of a tensor, without a device
        is_cuda, dtype, device = True, pkg.torch.uint8, "cpu"

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return 16

    class Lib:
        def icamd_encode_device(self, *a):
            calls.append(("encode", a))
            return 0

        def icamd_encode_etc2_colour_device(self, *a):
            calls.append(("colour", a))
            return 0

        def icamd_encoded_size(self, codec, gh, gw):
            return real.icamd_encoded_size(codec, gh, gw)

    monkeypatch.setattr(pkg, "lib", lambda: Lib())
    monkeypatch.setattr(pkg, "_stream_handle", lambda stream=None: None)
    out = pkg.torch.empty((1, 64), dtype=pkg.torch.uint8)
    pkg.encode_device(RGBA8, Tensor(), 8, 8, 4, out=out, etc_strategy=1, swap_rb=True, grid_height=12, row_stride_bytes=40)
    pkg.encode_etc2_colour_device(RGBA8, Tensor(), 8, 8, 4, out=out, etc_strategy=1, swap_rb=True, grid_height=12,
                                  row_stride_bytes=40)
    pkg.encode_etc2_colour_device(RGBA8, Tensor(), 8, 8, 4, out=out, etc_strategy=1, swap_rb=True, grid_height=12,
                                  row_stride_bytes=40, colour_modes=pkg.ETC2_COLOUR_PLANAR_TH)
    assert [c[0] for c in calls] == ["encode", "colour", "colour"]
    assert calls[1][1][:4] == (RGBA8, 1, 0, 4) and calls[1][1][4:] == calls[0][1][3:]
    assert calls[2][1][:4] == (RGBA8, 1, 2, 4) and calls[2][1][4:] == calls[0][1][3:]
    import inspect
    a, b = inspect.signature(pkg.encode_device).parameters, inspect.signature(pkg.encode_etc2_colour_device).parameters
    assert set(a) - {"etc2_modes"} == set(b) - {"colour_modes"}         # the keyword set of encode_device
    assert "etc2_modes" in a and a["etc2_modes"].default == 0            # encode_device keeps its keyword

