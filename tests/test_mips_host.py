"""CPU tier of the fused mip chain (include/ic_amd.h, mip-chain section):
* icamd_mip_max_levels / icamd_mip_chain_size / offsets / icamd_mip_workspace_size against a Python formula;
* every refusal returns its status, and valid arguments without a device fail loudly (no CPU path);
* the numpy pyramid of tests/mips_oracle.py against a literal restatement of the rule;
* a Python model of the pass plan (mip_plan.h) and the kernel's tile / level / edge index mapping (mip_pass.h) -- a restatement, not
  their code: tests/test_mip_plan_host.py holds the compiled plan against this model, and the GPU tier runs the kernels themselves on
  the same shapes -- against that pyramid;
* (ref) the compiled reference's Compress of every pyramid level equals the oracle's encode;
* the new kernels compile for gfx950 with zero scratch and the planned LDS size."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bc45_oracle as B
import ic_testlib as T
import mips_oracle as M

CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
ERR_ARG, FALSE = -4, 1
SHAPES = [(1, 1), (1, 7), (7, 1), (1, 4096), (4097, 1), (3, 5), (5, 3), (2, 3), (13, 1000), (1000, 13), (61, 59), (64, 64),
          (4097, 3), (128, 129), (255, 257), (4096, 4096), (16384, 16384), (1, 65535), (65535, 2)]


@pytest.fixture(scope="module")
def pkg():
    import ic_amd_loader
    return ic_amd_loader.load_package()


# ---- sizes and offsets

def test_max_levels_match_the_formula(pkg):
    for h, w in SHAPES + [(0, 5), (5, 0), (0xFFFFFFFF, 1), (2, 2), (3, 3), (4, 4)]:
        assert pkg.mip_max_levels(h, w) == M.max_levels(h, w), (h, w)
    assert pkg.mip_max_levels(4096, 4096) == 13 and pkg.mip_max_levels(16384, 16384) == 15


@pytest.mark.parametrize("codec", M.CODECS)
def test_chain_size_and_offsets_match_the_formula(pkg, codec):
    lib = pkg.lib()
    for h, w in SHAPES:
        top = M.max_levels(h, w)
        for levels in sorted({1, min(2, top), max(1, top // 2), top}):
            offs = (ctypes.c_size_t * (levels + 1))()
            n = lib.icamd_mip_chain_size(codec, h, w, levels, offs)
            want = M.chain_offsets(codec, h, w, levels)
            assert n == want[-1] and list(offs) == want, (codec, h, w, levels)
            assert lib.icamd_mip_chain_size(codec, h, w, levels, None) == want[-1]
            # each level's size is the existing icamd_encoded_size of that level
            for l in range(levels):
                assert want[l + 1] - want[l] == pkg.encoded_size(codec, *M.level_shape(h, w, l))
        assert lib.icamd_mip_chain_size(codec, h, w, 0, None) == 0
        assert lib.icamd_mip_chain_size(codec, h, w, top + 1, None) == 0
    for bad in (T.PVRTC2, 4, 7, -1):
        assert lib.icamd_mip_chain_size(bad, 64, 64, 3, None) == 0


def _workspace_formula(h, w, levels, comps, n):
    total, l0 = 0, 0
    while True:
        ih, iw = M.level_shape(h, w, l0)
        n_pass = levels - l0 if (ih <= 128 and iw <= 128) else min(levels - l0, 6)
        if l0 + n_pass >= levels:
            return total
        lh, lw = M.level_shape(h, w, l0 + 6)
        total += lh * lw * comps * n
        l0 += 6


def test_workspace_size(pkg):
    lib = pkg.lib()
    for h, w in SHAPES:
        for comps in (1, 2, 3, 4):
            top = M.max_levels(h, w)
            for levels in sorted({1, 6, 7, 12, 13, top}):
                if levels > top:
                    continue
                got = lib.icamd_mip_workspace_size(B.BC4, comps, h, w, levels, 3)
                assert got == _workspace_formula(h, w, levels, comps, 3), (h, w, comps, levels)
    assert lib.icamd_mip_workspace_size(T.DXT1, 4, 4096, 4096, 13, 1) == 64 * 64 * 4  # one handoff: level 6
    assert lib.icamd_mip_workspace_size(T.DXT1, 4, 16384, 16384, 15, 1) == 256 * 256 * 4 + 4 * 4 * 4  # levels 6 and 12
    assert lib.icamd_mip_workspace_size(T.DXT1, 4, 128, 128, 8, 1) == 0  # one tile: one pass
    # ETC1: the whole pixel pyramid (levels 1 .. levels-1) of every image
    for h, w in SHAPES[:12]:
        top = M.max_levels(h, w)
        want = sum(M.level_shape(h, w, l)[0] * M.level_shape(h, w, l)[1] * 3 for l in range(1, top)) * 2
        assert lib.icamd_mip_workspace_size(T.ETC1, 3, h, w, top, 2) == want, (h, w)


# ---- refusals (argument checks come before any device work)

def _enc(lib, codec=T.DXT1, comps=4, swap=0, h=64, w=64, stride=None, levels=7, n=1, sis=0, dis=0, src=16, dst=16,
         ws=None, ws_bytes=0):
    stride = w * comps if stride is None else stride
    return lib.icamd_encode_mips_device(codec, 2, comps, swap, h, w, stride, levels, n, sis, dis, src, dst, ws, ws_bytes, None)


def test_encode_refusals(pkg):
    lib = pkg.lib()
    assert _enc(lib, codec=T.PVRTC2) == ERR_ARG
    assert _enc(lib, codec=T.PVRTC4) == ERR_ARG
    assert _enc(lib, codec=9) == ERR_ARG
    assert _enc(lib, levels=0) == ERR_ARG
    assert _enc(lib, levels=8) == ERR_ARG  # 64 x 64 has 7
    assert _enc(lib, h=1, w=1, levels=2) == ERR_ARG
    assert _enc(lib, stride=64 * 4 - 1) == ERR_ARG
    assert _enc(lib, codec=T.DXT5, comps=3) == ERR_ARG
    assert _enc(lib, codec=T.DXT1, comps=2) == ERR_ARG
    assert _enc(lib, codec=T.ETC1, comps=1) == ERR_ARG
    assert _enc(lib, codec=B.BC5, comps=1) == ERR_ARG
    assert _enc(lib, codec=B.BC4, comps=5) == ERR_ARG
    assert _enc(lib, codec=B.BC4, comps=2, swap=1) == ERR_ARG
    # image strides smaller than an image (n_images > 1)
    chain = M.chain_offsets(T.DXT1, 64, 64, 7)[-1]
    assert _enc(lib, n=2, sis=64 * 64 * 4 - 1, dis=chain) == ERR_ARG
    assert _enc(lib, n=2, sis=64 * 64 * 4, dis=chain - 1) == ERR_ARG
    # a workspace that is too small (256^2: level 6 of 4 x 4 pixels is handed to a second pass)
    need = lib.icamd_mip_workspace_size(T.DXT1, 4, 256, 256, 9, 1)
    assert need == 4 * 4 * 4
    assert _enc(lib, h=256, w=256, levels=9) == ERR_ARG
    assert _enc(lib, h=256, w=256, levels=9, ws=64, ws_bytes=need - 1) == ERR_ARG
    # null pointers / empty images: ICAMD_FALSE, as icamd_encode_device
    assert _enc(lib, src=None) == FALSE
    assert _enc(lib, dst=None) == FALSE
    assert _enc(lib, h=0) == FALSE


def test_pyramid_and_host_refusals(pkg):
    lib = pkg.lib()
    pyr = lib.icamd_mip_pyramid_device
    assert pyr(0, 8, 8, 8, 2, 1, 0, 0, 16, 16, None) == ERR_ARG
    assert pyr(5, 8, 8, 40, 2, 1, 0, 0, 16, 16, None) == ERR_ARG
    assert pyr(4, 8, 8, 32, 0, 1, 0, 0, 16, 16, None) == ERR_ARG
    assert pyr(4, 8, 8, 32, 5, 1, 0, 0, 16, 16, None) == ERR_ARG
    assert pyr(4, 8, 8, 31, 2, 1, 0, 0, 16, 16, None) == ERR_ARG
    assert pyr(4, 8, 8, 32, 4, 2, 8 * 32, 16 * 4 + 4 * 4 + 4 - 1, 16, 16, None) == ERR_ARG
    assert pyr(4, 8, 8, 32, 2, 1, 0, 0, None, 16, None) == FALSE
    buf = np.zeros(64 * 64 * 4, np.uint8)
    out = np.zeros(1 << 16, np.uint8)
    cm = lib.icamd_compress_mips
    chain = M.chain_offsets(T.DXT5, 64, 64, 7)[-1]
    assert cm(T.PVRTC, 2, T.RGBA, 64, 64, 0, 7, buf.ctypes.data, out.ctypes.data, chain) == ERR_ARG
    assert cm(T.ETC, 2, T.RGBA, 64, 64, 0, 7, buf.ctypes.data, out.ctypes.data, chain) == FALSE  # ETC takes kRGB only
    assert cm(T.DXTC, 2, 9, 64, 64, 0, 7, buf.ctypes.data, out.ctypes.data, chain) == FALSE
    assert cm(T.DXTC, 2, T.RGBA, 64, 64, 0, 7, buf.ctypes.data, out.ctypes.data, chain - 1) == FALSE
    assert cm(T.DXTC, 2, T.RGBA, 64, 64, 0, 0, buf.ctypes.data, out.ctypes.data, chain) == ERR_ARG
    assert cm(T.DXTC, 2, T.RGBA, 64, 64, 0, 8, buf.ctypes.data, out.ctypes.data, chain) == ERR_ARG
    assert cm(T.DXTC, 2, T.RGBA, 64, 64, 0, 7, None, out.ctypes.data, chain) == FALSE


def test_no_gpu_means_a_loud_error_not_a_cpu_result(pkg):
    if pkg.lib().icamd_device_count() > 0:
        pytest.skip("a HIP device is present: the GPU tier covers this path")
    lib = pkg.lib()
    assert _enc(lib, h=256, w=256, levels=9, ws=64, ws_bytes=64) < 0
    assert lib.icamd_last_error().decode()
    assert lib.icamd_mip_pyramid_device(4, 8, 8, 32, 4, 1, 0, 0, 16, 16, None) < 0
    buf = np.zeros(64 * 64 * 3, np.uint8)
    out = np.zeros(1 << 16, np.uint8)
    chain = M.chain_offsets(T.DXT1, 64, 64, 7)[-1]
    assert lib.icamd_compress_mips(T.DXTC, 2, T.RGB, 64, 64, 0, 7, buf.ctypes.data, out.ctypes.data, chain) < 0
    with pytest.raises(pkg.BackendError):
        pkg.compress_mips_host(T.DXTC, T.RGB, buf, 64, 64)


# ---- the pyramid restatement

@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (9, 1), (2, 3), (3, 5), (5, 5), (7, 13), (13, 7), (17, 2), (33, 31)])
def test_numpy_pyramid_matches_the_literal_rule(h, w):
    rng = np.random.default_rng(h * 100 + w)
    for c in (1, 3, 4):
        p = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        levels = M.pyramid(p)
        assert len(levels) == M.max_levels(h, w)
        for l in range(1, len(levels)):
            assert levels[l].shape[:2] == M.level_shape(h, w, l)
            assert np.array_equal(levels[l], M.next_level_literal(levels[l - 1])), (h, w, c, l)
    # an odd side drops its last row / column: a bright last column never reaches level 1
    p = np.zeros((4, 5, 1), np.uint8)
    p[:, 4] = 255
    assert not M.next_level(p).any()
    # a side of 1 averages the pixel with itself
    p = np.array([[[10], [13]]], np.uint8)  # 1 x 2
    assert M.next_level(p)[0, 0, 0] == (10 + 13 + 10 + 13) // 4


# ---- a Python model of the kernel's index mapping (mip_plan.h's pass plan and mip_pass.h's 128 x 128 tiles, LDS levels and edge
# clamps, restated).  It checks the mapping's design -- that the tile rules reproduce the pyramid and the clamped blocks on odd, thin and
# multi-tile shapes -- not the compiled code, which tests/test_gpu_mips.py checks on the device.

def _model_plan(h, w, levels, pyramid):
    plan, l0 = [], 0
    while True:
        ih, iw = M.level_shape(h, w, l0)
        single = ih <= 128 and iw <= 128
        n = levels - l0 if single else min(levels - l0, 7 if pyramid else 6)
        plan.append((l0, n, ih, iw, l0 + n < levels))
        if l0 + n >= levels:
            return plan
        l0 += 6


def _avg4(a, b, c, d):
    return ((a.astype(np.uint16) + b + c + d) // 4).astype(np.uint8)


def _model_pass(src, n, enc_levels, pix_levels):
    """One launch over an input level `src` (ih, iw, c): returns {j: block pixel arrays (by, bx, 4, 4, c)} for the encoded
    local levels and {j: pixel image} for the pixel outputs, built tile by tile exactly as the kernel indexes them."""
    ih, iw, c = src.shape
    jmax = max([j for j in enc_levels + pix_levels if j >= 1], default=0)
    blocks = {j: np.zeros(((M.level_shape(ih, iw, j)[0] + 3) // 4, (M.level_shape(ih, iw, j)[1] + 3) // 4, 4, 4, c), np.uint8)
              for j in enc_levels}
    pix = {j: np.zeros(M.level_shape(ih, iw, j) + (c,), np.uint8) for j in pix_levels}
    for ty in range((ih + 127) // 128):
        for tx in range((iw + 127) // 128):
            def lvl(j):
                lh, lw = M.level_shape(ih, iw, j)
                side = 128 >> j
                x0, y0 = tx * side, ty * side
                return lw, lh, x0, y0, min(side, lw - x0), min(side, lh - y0)
            lds = {}
            if jmax:
                lds[1] = np.zeros((64, 64, c), np.uint8)
            for i in range(1024):  # level 0: four rounds of 256 lanes
                bx, by = i & 31, i >> 5
                row, col = (ty * 32 + by) * 4, (tx * 32 + bx) * 4
                if row >= ih or col >= iw:
                    continue
                ys = np.minimum(row + np.arange(4), ih - 1)
                xs = np.minimum(col + np.arange(4), iw - 1)
                px = src[ys][:, xs]
                if jmax:
                    lds[1][2 * by:2 * by + 2, 2 * bx:2 * bx + 2] = _avg4(px[0::2, 0::2], px[0::2, 1::2], px[1::2, 0::2], px[1::2, 1::2])
                if 0 in enc_levels:
                    blocks[0][row >> 2, col >> 2] = px
            for j in range(2, jmax + 1):
                _, _, _, _, vw, vh = lvl(j - 1)
                sx, sy = (1 if vw >= 2 else 0), (1 if vh >= 2 else 0)
                s = 128 >> j
                prev = lds[j - 1]
                yy, xx = 2 * np.arange(s), 2 * np.arange(s)
                lds[j] = _avg4(prev[yy][:, xx], prev[yy][:, xx + sx], prev[yy + sy][:, xx], prev[yy + sy][:, xx + sx])
            for j in pix_levels:
                lw, lh, x0, y0, vw, vh = lvl(j)
                pix[j][y0:y0 + vh, x0:x0 + vw] = lds[j][:vh, :vw]
            for j in enc_levels:
                if j == 0:
                    continue
                lw, lh, x0, y0, vw, vh = lvl(j)
                nb = max(1, (128 >> j) // 4)
                for by in range(nb):
                    for bx in range(nb):
                        if bx * 4 >= vw or by * 4 >= vh:
                            continue
                        ys = np.minimum(by * 4 + np.arange(4), vh - 1)
                        xs = np.minimum(bx * 4 + np.arange(4), vw - 1)
                        blocks[j][(y0 >> 2) + by, (x0 >> 2) + bx] = lds[j][ys][:, xs]
    return blocks, pix


def _clamped_blocks(p):
    h, w, c = p.shape
    bh, bw = (h + 3) // 4, (w + 3) // 4
    ys = np.minimum(np.arange(bh * 4), h - 1)
    xs = np.minimum(np.arange(bw * 4), w - 1)
    return p[ys][:, xs].reshape(bh, 4, bw, 4, c).transpose(0, 2, 1, 3, 4)


@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (5, 5), (13, 300), (300, 13), (1, 517), (517, 1), (61, 59), (128, 128),
                                 (129, 127), (200, 600), (256, 256), (257, 255), (1024, 3), (3, 1024)])
def test_python_model_of_the_tile_mapping(h, w):
    rng = np.random.default_rng(h * 7919 + w)
    c = 2
    img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    levels = M.max_levels(h, w)
    want = M.pyramid(img, levels)
    # fused encode: every level's blocks see exactly the clamped blocks of the numpy pyramid level
    src = img
    for l0, n, ih, iw, handoff in _model_plan(h, w, levels, False):
        assert src.shape[:2] == (ih, iw)
        blocks, pix = _model_pass(src, n, list(range(n)), [6] if handoff else [])
        for j in range(n):
            assert np.array_equal(blocks[j], _clamped_blocks(want[l0 + j])), (h, w, l0 + j)
        if handoff:
            src = pix[6]
    # pixel pyramid: levels 1 .. levels-1, the last of each pass the next pass's input
    src = img
    for l0, n, ih, iw, handoff in _model_plan(h, w, levels, True):
        _, pix = _model_pass(src, n, [], list(range(1, n)))
        for j in range(1, n):
            assert np.array_equal(pix[j], want[l0 + j]), (h, w, l0 + j)
        if handoff:
            src = pix[6]


# ---- the oracle's level encode against the compiled reference (build container only)

@pytest.mark.ref
@pytest.mark.skipif(not T.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (5, 5), (13, 70), (70, 13), (1, 33), (61, 59), (64, 64), (128, 32)])
def test_pyramid_levels_pinned_to_the_reference(h, w):
    for compressor, fmt, codec, comps in [(T.DXTC, T.RGB, T.DXT1, 3), (T.DXTC, T.RGBA, T.DXT5, 4), (T.ETC, T.RGB, T.ETC1, 3),
                                          (T.DXTC, T.BGR, T.DXT1, 3)]:
        img = T.s_mixed(h, w, comps, index=h + w).reshape(h, w, comps)
        swap = 1 if fmt == T.BGR else 0
        for l, p in enumerate(M.pyramid(img)):
            lh, lw = p.shape[:2]
            ref = T.ref_compress(compressor, fmt, np.ascontiguousarray(p), lh, lw)
            assert ref == M.oracle_encode(codec, p, comps, swap), (h, w, codec, l)


# ---- build check: zero scratch, the planned LDS

def test_mip_kernels_use_no_scratch_and_the_planned_lds(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path), "k.s")
    subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(T.ROOT, "include"),
                           "-I" + CSRC, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "mip_kernels.hip")],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    metas = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        metas[name] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                       int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)))
    names = [n for n in metas if n.startswith("icamd_mip_")]
    assert len(names) == 14, sorted(metas)  # DXT1 x 2, DXT5, BC4 x 4, BC5 x 3, pyramid x 4
    pyramid_lds = 5461 * 4  # levels 1..7 of a 128 x 128 tile as pixel dwords
    for n in names:
        scratch, lds = metas[n]
        assert scratch == 0, "%s uses %d bytes of scratch" % (n, scratch)
        # + the DXT colour search's per-lane 64-byte stash (dxt_block.h BlockStash)
        # (the stash's 16-byte alignment rounds the pyramid's 21 844 bytes up to 21 856)
        want = (-(-pyramid_lds // 16) * 16 + 256 * 64) if ("dxt1" in n or "dxt5" in n) else pyramid_lds
        assert lds == want, (n, lds)
